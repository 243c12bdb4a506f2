"""Seeded meshes and rays for the ray-casting tests (tests/test_mesh_host.py, tests/test_mesh_rays.py), the float64 oracle
and the numpy fp32 restatement of the kernels' formula (miso_amd/csrc/mesh.hpp: RayBest::take).

Oracle: all-triangles Moller-Trumbore in numpy float64, two-sided; a hit iff det != 0, u >= 0, v >= 0, u + v <= 1 and
t_min <= t <= t_max; the winner is the smallest (t, triangle index).  A triangle with a non-finite vertex or with
(v1 - v0) x (v2 - v0) == 0 is never hit (the fixtures' zero-area triangles have two equal vertices or exactly collinear
dyadic ones, so float64 and fp32 agree on which they are).

Ill-conditioned rays are left out of the float64 comparison (never out of the route-equality test): a ray for which some
triangle with 0 <= t64 <= t_best64 (1 + 1e-6) has |min(u, v, 1 - u - v)| < 1e-4, or hits with |det| / (|e1 x e2| |d|) <
1e-3.  At most KEPT_CAP of a fixture's rays may go.  `lattice` is exact in fp32 (integer vertices, dyadic origins,
directions in {0, +-1}^3): every one of its rays is kept, its edge and vertex rays are the point.

Tolerance on t: e = |t - t64| |d| / (max |coordinate| + t64 |d|), max |coordinate| over the fixture's hittable vertices
and finite ray origins.  Its maximum over the kept rays of all fixtures under the numpy fp32 restatement (cast_fp32
below, on the CPU) is FP32_E_MAX; a kernel may differ from numpy by an ulp per operation in its division and its order,
so it gets T_TOL = 4 FP32_E_MAX.  Measured with
    python -c "import sys; sys.path.insert(0, 'tests'); import mesh_cases as m; print(m.measure_fp32_error())"
which printed 5.17e-06 = 87 * 2^-24 (worst fixture: sliver, whose 3 cm triangles sit at coordinates of metres: the error of
u, v and t scales with the coordinates over the triangle's size; room 1.7e-07, open 6.8e-08, straddle 6.6e-08, lattice 0)."""
import functools

import numpy as np

KEPT_CAP = 0.01
FP32_E_MAX = 5.18e-06
T_TOL = 4.0 * FP32_E_MAX


# ---- the formula ---------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return np.stack((a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]), axis=-1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def hittable(vertices, triangles, dtype=np.float64):
    """bool (T,): finite vertices and a non-zero cross product in ``dtype``"""
    v = np.asarray(vertices, dtype=dtype)[np.asarray(triangles)]
    with np.errstate(all="ignore"):
        n = _cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        return np.isfinite(v).all(axis=(1, 2)) & np.isfinite(n).all(axis=1) & (n != 0).any(axis=1)


def _all_triangles(origins, dirs, vertices, triangles, dtype, chunk=256):
    """per chunk of rays: (t, u, v, det, hit-with-any-t) of every (ray, triangle), in ``dtype`` with numpy's one rounding per op"""
    v = np.asarray(vertices, dtype=dtype)[np.asarray(triangles)]
    ok = hittable(vertices, triangles, dtype)
    v0, e1, e2 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    o_all, d_all = np.asarray(origins, dtype=dtype), np.asarray(dirs, dtype=dtype)
    for a in range(0, len(o_all), chunk):
        o, d = o_all[a:a + chunk, None, :], d_all[a:a + chunk, None, :]
        with np.errstate(all="ignore"):
            p = _cross(d, e2[None])
            det = _dot(e1[None], p)
            inv = dtype(1.0) / det
            s = o - v0[None]
            u = _dot(s, p) * inv
            q = _cross(s, e1[None])
            w = _dot(d, q) * inv
            t = _dot(e2[None], q) * inv
            inside = ok[None] & (det != 0) & (u >= 0) & (w >= 0) & (u + w <= 1)
        yield slice(a, a + chunk), t, u, w, det, inside, (e1, e2, d)


def _cast(origins, dirs, vertices, triangles, t_min, t_max, dtype):
    n = len(origins)
    out = {k: np.full(n, np.nan, dtype=dtype) for k in ("u", "v", "det")}
    out["t"] = np.full(n, np.inf, dtype=dtype)
    out["tri"] = np.full(n, -1, dtype=np.int64)
    if len(triangles) == 0 or n == 0:
        return out
    for sl, t, u, w, det, inside, _ in _all_triangles(origins, dirs, vertices, triangles, dtype):
        with np.errstate(all="ignore"):
            hit = inside & (t >= t_min) & (t <= t_max)
        tt = np.where(hit, t, np.inf)
        first = np.argmin(tt, axis=1)                      # the lowest index among equal t
        rows = np.arange(tt.shape[0])
        got = hit[rows, first]
        out["t"][sl] = np.where(got, tt[rows, first], np.inf)
        out["tri"][sl] = np.where(got, first, -1)
        for k, arr in (("u", u), ("v", w), ("det", det)):
            out[k][sl] = np.where(got, arr[rows, first], np.nan)
    return out


def oracle(origins, dirs, vertices, triangles, t_min=0.0, t_max=np.inf):
    """float64: {'t', 'tri', 'u', 'v', 'det'} of the winner per ray; (+inf, -1, nan, nan, nan) for a miss"""
    return _cast(origins, dirs, vertices, triangles, t_min, t_max, np.float64)


def cast_fp32(origins, dirs, vertices, triangles, t_min=0.0, t_max=np.inf):
    """the kernels' formula in numpy float32 (inputs rounded to fp32 first, as the device sees them)"""
    f = np.float32
    return _cast(np.asarray(origins, f), np.asarray(dirs, f), np.asarray(vertices, f), triangles, f(t_min), f(t_max), f)


def kept_rays(origins, dirs, vertices, triangles, best_t):
    """bool (N,): the rays that stay in the float64 comparison (module docstring); ``best_t`` the oracle's t"""
    keep = np.ones(len(origins), dtype=bool)
    if len(triangles) == 0:
        return keep
    for sl, t, u, w, det, inside, (e1, e2, d) in _all_triangles(origins, dirs, vertices, triangles, np.float64):
        with np.errstate(all="ignore"):
            near = (t >= 0) & (t <= best_t[sl, None] * (1 + 1e-6))
            edge = np.abs(np.minimum(np.minimum(u, w), 1 - u - w)) < 1e-4
            area = np.linalg.norm(_cross(e1, e2), axis=1)[None]
            graze = inside & (np.abs(det) / (area * np.linalg.norm(d, axis=2)) < 1e-3)
            keep[sl] &= ~(near & (edge | graze)).any(axis=1)
    return keep


# ---- meshes ----------------------------------------------------------------------------------------------------------------
def box(lo, hi):
    """twelve triangles of the box [lo, hi] -> (vertices (8, 3), triangles (12, 3))"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    v = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=np.int64)


def height_field(rng, n, lo, hi, z0, bump):
    """an n x n bumpy height field over [lo, hi]^2 at height about z0"""
    xs, ys = np.linspace(lo[0], hi[0], n), np.linspace(lo[1], hi[1], n)
    X, Y = np.meshgrid(xs, ys, indexing="ij")
    Z = z0 + bump * rng.standard_normal((n, n))
    v = np.stack([X, Y, Z], axis=-1).reshape(-1, 3)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    return v, np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int64)


def join(parts):
    vs, ts, at = [], [], 0
    for v, t in parts:
        vs.append(np.asarray(v, float)); ts.append(np.asarray(t, np.int64) + at); at += len(v)
    return np.concatenate(vs), np.concatenate(ts)


def small_triangles(rng, n, lo, hi, size):
    c = rng.uniform(lo, hi, size=(n, 1, 3))
    v = (c + size * rng.standard_normal((n, 3, 3))).reshape(-1, 3)
    return v, np.arange(3 * n, dtype=np.int64).reshape(n, 3)


def unit_dirs(rng, n):
    d = rng.standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _fixture(name, vertices, triangles, origins, dirs, cells):
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32))          # noqa: E731
    return {"name": name, "vertices": f32(vertices), "triangles": np.ascontiguousarray(triangles, dtype=np.int64),
            "origins": f32(origins), "dirs": f32(dirs), "cells": cells}


def room(seed=7, n_rays=4096):
    """an 8 x 6 x 3 box (12 huge triangles) around a 25 x 25 bumpy height field and 300 small triangles: 1 464 triangles"""
    rng = np.random.default_rng(seed)
    v, t = join([box((0, 0, 0), (8, 6, 3)), height_field(rng, 25, (0.5, 0.5), (7.5, 5.5), 0.8, 0.08),
                 small_triangles(rng, 300, (0.5, 0.5, 1.2), (7.5, 5.5, 2.8), 0.05)])
    o = rng.uniform((0.3, 0.3, 1.1), (7.7, 5.7, 2.9), size=(n_rays, 3))
    return _fixture("room", v, t, o, unit_dirs(rng, n_rays) * rng.uniform(0.5, 2.0, size=(n_rays, 1)), (0.11, 1.7))


def open_field(seed=11, n_rays=2048):
    """the height field alone, rays from above and below over a wider footprint: about half miss"""
    rng = np.random.default_rng(seed)
    v, t = height_field(rng, 25, (0.0, 0.0), (4.0, 4.0), 0.0, 0.05)
    o = rng.uniform((-0.9, -0.9, 1.0), (4.9, 4.9, 2.0), size=(n_rays, 3))
    o[::2, 2] *= -1.0
    d = 0.15 * rng.standard_normal((n_rays, 3))
    d[:, 2] = -np.sign(o[:, 2])
    return _fixture("open", v, t, o, d, (0.09, 1.3))


def lattice():
    """unit quads on integer planes of [0, 4]^3, dyadic origins, directions in {0, +-1}^3: every t is exact in fp32"""
    quads = []

    def quad(axis, k, a, b):
        p = [None] * 4
        for i, (da, db) in enumerate(((0, 0), (1, 0), (1, 1), (0, 1))):
            c = [0, 0, 0]
            c[axis], c[(axis + 1) % 3], c[(axis + 2) % 3] = k, a + da, b + db
            p[i] = c
        quads.append(p)

    for axis in range(3):
        for k in (0, 4):
            for a in range(4):
                for b in range(4):
                    quad(axis, k, a, b)
        for a in (1, 2):                                   # an inner wall of 2 x 2 quads on the plane 2
            for b in (1, 2):
                quad(axis, 2, a, b)
    v = np.array(quads, dtype=float).reshape(-1, 3)
    idx = np.arange(len(v)).reshape(-1, 4)
    t = np.concatenate([idx[:, [0, 1, 2]], idx[:, [0, 2, 3]]], axis=1).reshape(-1, 3)
    dirs = np.array([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], float)
    # origins: inside on quarter points (faces, edges and corners of the cells of 1 and of 0.5 among them) and outside the grid
    g = np.arange(0.25, 4.0, 0.25)
    inner = np.array([[x, y, z] for x in g[::3] for y in g[1::3] for z in g[2::3]])
    faces = np.array([[1.0, 1.5, 2.5], [1.0, 2.0, 2.5], [1.0, 2.0, 3.0], [3.0, 3.0, 3.0], [0.5, 1.0, 1.0], [2.5, 0.5, 3.0],
                      [1.0, 1.0, 1.0], [3.0, 1.0, 2.0], [1.5, 1.5, 1.5], [0.0, 0.0, 0.0], [4.0, 2.0, 2.0], [2.0, 2.0, 2.0]])
    outer = np.array([[-1.0, 1.5, 1.5], [5.0, 2.0, 2.0], [-2.0, -2.0, -2.0], [6.0, 6.0, 1.0], [1.0, -3.0, 1.0], [2.25, 2.75, 9.0],
                      [-1.0, -1.0, 1.0], [5.0, 5.0, 5.0], [2.0, 2.0, -4.0]])
    o = np.concatenate([inner, faces, outer])
    O = np.repeat(o, len(dirs), axis=0)
    D = np.tile(dirs, (len(o), 1))
    return _fixture("lattice", v, t, O, D, (0.5, 1.0))


def straddle(seed=3, n_rays=2048, cell=0.37):
    """bounds from about -75.14 to 75 (flat in z), small triangles lying in planes within ulps of cell faces, rays across"""
    rng = np.random.default_rng(seed)
    f = np.float32
    lo = f(-75.14)
    n = 400
    k = rng.integers(1, int(150.0 / cell) - 1, size=n)
    plane = (lo + (k.astype(f) * f(cell))).astype(f)                   # the kernels' face k, in their arithmetic
    ulps = rng.integers(-3, 4, size=n)
    x = plane.copy()
    for _ in range(3):
        x = np.where(ulps > 0, np.nextafter(x, f(np.inf)), np.where(ulps < 0, np.nextafter(x, f(-np.inf)), x))
        ulps = ulps - np.sign(ulps)
    c = np.stack([x.astype(float), rng.uniform(-70, 70, n), rng.uniform(0.5, 2.5, n)], axis=1)
    axis = rng.integers(0, 2, size=n)                                  # the face is an x face or a y face
    tri = np.zeros((n, 3, 3))
    for i in range(n):
        a, b = int(axis[i]), 1 - int(axis[i])
        centre = c[i].copy()
        if a == 1:
            centre[0], centre[1] = c[i][1], c[i][0]
        for j, (du, dv) in enumerate(((-0.3, -0.2), (0.3, -0.2), (0.0, 0.3))):
            p = centre.copy()
            p[b] += du
            p[2] += dv
            tri[i, j] = p
    corners = np.array([[-75.14, -75.14, 0.0], [-75.14, -75.0, 0.0], [-75.0, -75.14, 0.1],
                        [75.0, 75.0, 3.0], [75.0, 74.9, 3.0], [74.9, 75.0, 2.9]])
    v = np.concatenate([tri.reshape(-1, 3), corners])
    t = np.arange(len(v), dtype=np.int64).reshape(-1, 3)
    # rays: from a point off a triangle's face through a point of the triangle, and beyond
    pick = rng.integers(0, n, size=n_rays)
    w = rng.dirichlet((1.0, 1.0, 1.0), size=n_rays)
    target = (tri[pick] * w[:, :, None]).sum(axis=1)
    off = rng.uniform(-1.0, 1.0, size=(n_rays, 3)) * (3.0, 3.0, 0.3)
    far = rng.random(n_rays) < 0.3
    off[far] *= 30.0
    o = target + off
    o[:, 2] = np.clip(o[:, 2], 0.05, 2.95)
    d = (target - o) * rng.uniform(0.3, 1.5, size=(n_rays, 1))
    return _fixture("straddle", v, t, o, d, (cell, 7.9))


def sliver(seed=5, n_rays=2048):
    """one triangle across the whole grid diagonal beside many tiny ones; zero-area, NaN and duplicated triangles"""
    rng = np.random.default_rng(seed)
    big = (np.array([[0.0, 0.0, 0.0], [6.0, 6.0, 4.0], [6.0, 5.5, 4.0]]), np.array([[0, 1, 2]]))
    tiny = small_triangles(rng, 500, (0.2, 0.2, 0.2), (5.8, 5.8, 3.8), 0.03)
    dup = (tiny[0][:60], tiny[1][:20])                                  # the first twenty again: the lower index wins
    zero = (np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [2.0, 1.0, 1.5],            # two equal vertices
                      [1.0, 2.0, 1.0], [2.0, 3.0, 1.5], [3.0, 4.0, 2.0]]),          # collinear, dyadic
            np.array([[0, 1, 2], [3, 4, 5]]))
    bad = (np.array([[2.0, 2.0, 2.0], [np.nan, 2.0, 2.0], [2.0, 3.0, 2.0], [1.0, 1.0, 3.0], [np.inf, 1.0, 3.0], [1.0, 2.0, 3.0]]),
           np.array([[0, 1, 2], [3, 4, 5]]))
    v, t = join([big, tiny, dup, zero, bad])
    o = rng.uniform((0.1, 0.1, 0.1), (5.9, 5.9, 3.9), size=(n_rays, 3))
    d = unit_dirs(rng, n_rays)
    aim = rng.random(n_rays) < 0.5                                      # half the rays aim at a tiny triangle
    centres = tiny[0].reshape(-1, 3, 3).mean(axis=1)
    d[aim] = centres[rng.integers(0, len(centres), size=int(aim.sum()))] - o[aim]
    return _fixture("sliver", v, t, o, d, (0.07, 1.1))


FIXTURES = {"room": room, "open": open_field, "lattice": lattice, "straddle": straddle, "sliver": sliver}


@functools.lru_cache(maxsize=None)
def fixture(name):
    """the fixture with its oracle: adds 'ref' (float64, over the fp32 inputs as the device sees them), 'kept', 'coord_max'"""
    fx = dict(FIXTURES[name]())
    fx["ref"] = oracle(fx["origins"], fx["dirs"], fx["vertices"], fx["triangles"])
    if name == "lattice":
        fx["kept"] = np.ones(len(fx["origins"]), dtype=bool)
    else:
        fx["kept"] = kept_rays(fx["origins"], fx["dirs"], fx["vertices"], fx["triangles"], fx["ref"]["t"])
    ok = hittable(fx["vertices"], fx["triangles"])
    used = fx["vertices"][fx["triangles"][ok]].astype(np.float64)
    fx["coord_max"] = float(max(np.abs(used).max(), np.abs(fx["origins"][np.isfinite(fx["origins"]).all(axis=1)]).max()))
    return fx


def t_error(fx, t):
    """e of the module docstring for every ray whose float64 answer is a hit (nan elsewhere)"""
    ref = fx["ref"]["t"]
    dn = np.linalg.norm(fx["dirs"].astype(np.float64), axis=1)
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(ref), np.abs(np.asarray(t, np.float64) - ref) * dn / (fx["coord_max"] + ref * dn), np.nan)


def measure_fp32_error():
    """max e over the kept rays of all fixtures under cast_fp32: the figure behind FP32_E_MAX"""
    worst = {}
    for name in FIXTURES:
        fx = fixture(name)
        got = cast_fp32(fx["origins"], fx["dirs"], fx["vertices"], fx["triangles"])
        e = t_error(fx, got["t"])[fx["kept"]]
        worst[name] = float(np.nanmax(e)) if np.isfinite(e).any() else 0.0
    return max(worst.values()), worst


# ---- the grid route restated: lists and walk of miso_amd/csrc/mesh.hip in numpy fp32 ------------------------------------------
def mesh_plan(vertices, triangles, cell):
    """miso_mesh_plan (host logic of the library) over the hittable triangles' bounds -> the plan struct"""
    import ctypes
    from miso_amd import _lib
    ok = hittable(vertices, triangles, np.float32)
    used = np.asarray(vertices, np.float32)[np.asarray(triangles)[ok]].reshape(-1, 3)
    plan = _lib.MeshPlan()
    lo, hi = (used.min(axis=0), used.max(axis=0)) if len(used) else (np.zeros(3), np.zeros(3))
    rc = _lib.load().miso_mesh_plan((ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*hi), float(cell), int(ok.sum() and len(triangles)),
                                    ctypes.byref(plan))
    assert rc == 0, rc
    return plan


def walk_fp32(vertices, triangles, origins, dirs, plan, slack=True, t_min=0.0, t_max=np.inf, max_candidates=32):
    """The grid route on the CPU, every operation in numpy float32 as the kernels order them: which cells list a triangle
    (its box in cell coordinates widened by w, and the plane-slab test), the clip to the widened box, the start cell, the
    walk with its per-step boundaries and its stop rule.  ``slack=False`` is the bare rule: w = 0 everywhere.
    Per ray the candidates are its hits of the all-triangles pass (the nearest ``max_candidates``); a candidate counts once
    the walk visits a cell that lists it.  -> (t, tri, t_all, tri_all): the walk's answer and the all-triangles answer."""
    f = np.float32
    tri = np.asarray(triangles)
    lo, cell = np.array(list(plan.bound_min), f), f(plan.cell)
    dims = np.array(list(plan.dims), np.int64)
    w = f(plan.widen) if slack else f(0.0)
    with np.errstate(all="ignore"):
        v = np.asarray(vertices, f)[tri]
        ok = hittable(vertices, tri, f)
        v0, e1, e2 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]

        def cell_axis(p):
            return np.clip(np.nan_to_num(np.floor((p - lo) / cell), nan=0.0), 0, (dims - 1).astype(f)).astype(np.int64)

        p1, p2 = v0 + e1, v0 + e2
        c_lo = cell_axis(np.minimum(v0, np.minimum(p1, p2)) - w)
        c_hi = cell_axis(np.maximum(v0, np.maximum(p1, p2)) + w)
        n = _cross(e1, e2)
        l1 = (np.abs(e1[:, 0]) + np.abs(e1[:, 1])) + np.abs(e1[:, 2])
        l2 = (np.abs(e2[:, 0]) + np.abs(e2[:, 1])) + np.abs(e2[:, 2])
        reach = (f(0.5) * cell + f(2.0) * w) * ((np.abs(n[:, 0]) + np.abs(n[:, 1])) + np.abs(n[:, 2])) * (f(1.0) + f(2.0 ** -10)) + \
            f(2.0 ** -20) * (l1 * l2) * ((l1 + l2) + f(2.0) * cell)
        o, d = np.asarray(origins, f), np.asarray(dirs, f)
        R = len(o)
        K = min(len(tri), max_candidates)
        tK, iK = np.full((R, K), np.inf, f), np.zeros((R, K), np.int64)
        for sl, t, u, q, det, inside, _ in _all_triangles(o, d, vertices, tri, f):
            tt = np.where(inside & (t >= f(t_min)) & (t <= f(t_max)), t, f(np.inf))
            order = np.argsort(tt, axis=1, kind="stable")[:, :K]
            tK[sl], iK[sl] = np.take_along_axis(tt, order, axis=1), order
        inv = np.where(d != 0, f(1.0) / d, f(0.0)).astype(f)
        step = np.sign(d).astype(np.int64)
        lo_w, hi_w = lo - w, (lo + dims.astype(f) * cell) + w
        ta, tb = (lo_w - o) * inv, (hi_w - o) * inv
        nz = d != 0
        t0 = np.maximum(f(t_min), np.where(nz, np.minimum(ta, tb), f(-np.inf)).max(axis=1)).astype(f)
        t1 = np.minimum(f(t_max), np.where(nz, np.maximum(ta, tb), f(np.inf)).min(axis=1)).astype(f)
        covered = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (np.abs(o) <= f(4.0) * f(plan.coord_mag)).all(axis=1)
        assert covered.all(), "walk_fp32 restates the walk only (a ray outside its guarantee reads all rows)"
        miss = (~nz & ((o < lo_w) | (o > hi_w))).any(axis=1) | ~nz.any(axis=1)
        active = ~miss & (t0 <= t1)
        c = cell_axis(o + t0[:, None] * d)
        found = np.zeros((R, K), bool)
        best_t = np.full(R, np.inf, f)
        rows = np.arange(R)
        for _ in range(int(dims.sum()) + 3):
            if not active.any():
                break
            cc = c[:, None, :]
            centre = lo + (c.astype(f) + f(0.5)) * cell
            rel = centre[:, None, :] - v0[iK]
            listed = ok[iK] & ((c_lo[iK] <= cc) & (cc <= c_hi[iK])).all(axis=2) & ~(np.abs(_dot(n[iK], rel)) > reach[iK])
            found |= listed & active[:, None] & np.isfinite(tK)
            best_t = np.where(found, tK, f(np.inf)).min(axis=1)
            ahead = (c + (step > 0)).astype(f)
            tm = np.where(step == 0, f(np.inf), ((lo + ahead * cell) - o) * inv).astype(f)
            t_out = tm.min(axis=1)
            active &= ~((best_t < t_out) | (t_out > t1) | ~(t_out < f(np.inf)))
            a = np.argmax(tm == t_out[:, None], axis=1)
            c[rows[active], a[active]] += step[rows[active], a[active]]
            active &= ((c >= 0) & (c < dims)).all(axis=1)
            c = np.clip(c, 0, dims - 1)
        first = np.argmax(found, axis=1)                       # candidates are sorted by (t, index)
        got = found[rows, first]
        return (np.where(got, tK[rows, first], f(np.inf)), np.where(got, iK[rows, first], -1),
                tK[:, 0], np.where(np.isfinite(tK[:, 0]), iK[:, 0], -1))
