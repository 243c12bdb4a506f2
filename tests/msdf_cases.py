"""Seeded meshes and queries for the mesh-distance tests (tests/test_mesh_sdf_host.py, tests/test_mesh_sdf.py), the float64
oracles and the numpy fp32 restatements of the kernels (miso_amd/csrc/mesh.hpp: TriBest::take, mesh_ring_finished,
mesh_walk_ray with RayCount; miso_amd/csrc/mesh_sdf.hip: the two-level shell walk).  Meshes come from mesh_cases.

Oracle, distance: all triangles in numpy float64, the closest point of each by the region-classified form the kernels use
(three vertex regions, three edge regions, interior), the winner the smallest (d2, triangle index).  A triangle with a
non-finite vertex or a zero cross product is never the answer.  Oracle, crossings: mesh_cases' Moller-Trumbore, the number
of triangles that pass its hit test.

Tolerance on d: e = |d - d64| / (max |coordinate| + d64), max |coordinate| over the fixture's hittable vertices and finite
queries.  Its maximum over all fixtures under the numpy fp32 restatement (closest_fp32 below, on the CPU) is FP32_E_MAX; a
kernel may differ from numpy by an ulp per operation in its division and its order, so it gets D_TOL = 4 FP32_E_MAX, the
project's margin.  The winning triangle may differ from float64's only where its own d64 is within D_TOL of the best.
Measured with
    python -c "import sys; sys.path.insert(0, 'tests'); import msdf_cases as m; print(m.measure_fp32_error())"
which printed 7.59e-07 (worst fixture: sliver, whose long thin triangle loses digits of the interior barycentrics to the
cancellation in va, vb, vc; nested 4.6e-08, open 1.2e-08, straddle 1.0e-08, room 2.3e-09, far 9.6e-11, cube 0).

Signs and counts against float64: a ray is kept by mesh_cases.kept_rays' conditioning rule over ALL its hits (best_t =
+inf: no triangle in front of the origin is hit within 1e-4 of its border or at a grazing angle), a point when all three
of its parity rays are; at most KEPT_CAP of a fixture's points may go (checked on the CPU with the oracle alone; the seeded
fixtures lose at most 0.26 %).  `cube` is outside that cap by design: its lattice puts 15 % of its points ON faces, edges and
vertices, where the distance is exact and the side is anybody's; its signs are compared off the surface.  Route equality
is asserted on all points, never filtered."""
import functools

import numpy as np

import mesh_cases as mc

KEPT_CAP = 0.01
FP32_E_MAX = 7.6e-07
D_TOL = 4.0 * FP32_E_MAX

# ops.MESH_PARITY_DIRS restated (the host test compares the two)
PARITY_DIRS = np.array([[2.0 / 7.0, 3.0 / 7.0, 6.0 / 7.0], [-9.0 / 11.0, 6.0 / 11.0, 2.0 / 11.0], [-4.0 / 9.0, -8.0 / 9.0, 1.0 / 9.0]])


# ---- the formula -----------------------------------------------------------------------------------------------------------
def tri_point(q, v0, e1, e2):
    """TriBest::take's arithmetic on broadcastable (..., 3) arrays of one dtype, operation for operation -> (d2, v, w)"""
    dt = q.dtype.type
    zero, one = dt(0), dt(1)
    dot = mc._dot
    with np.errstate(all="ignore"):
        ap = q - v0
        bp, cp = ap - e1, ap - e2
        d1, d2, d3, d4, d5, d6 = dot(e1, ap), dot(e2, ap), dot(e1, bp), dot(e2, bp), dot(e1, cp), dot(e2, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        regions = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                   (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
        w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = one / ((va + vb) + vc)
        v_in = np.fmin(np.fmax(vb * den, zero), one)                       # fmaxf(NaN, 0) = 0, as on the device
        w_in = np.fmin(np.fmax(vc * den, zero), one - v_in)
        full = lambda x: np.broadcast_to(np.asarray(x, dtype=dt), d1.shape)            # noqa: E731
        v = np.select(regions, [full(zero), full(one), d1 / (d1 - d3), full(zero), full(zero), one - w_bc], v_in).astype(dt)
        w = np.select(regions, [full(zero), full(zero), full(zero), full(one), d2 / (d2 - d6), w_bc], w_in).astype(dt)
        r = ap - (v[..., None] * e1 + w[..., None] * e2)
        return (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2], v, w


def _rows(vertices, triangles, dtype):
    """v0, e1, e2 as the kernels' rows hold them, and which triangles can be the answer"""
    v = np.asarray(vertices, dtype=dtype)[np.asarray(triangles)]
    with np.errstate(all="ignore"):
        return v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], mc.hittable(vertices, triangles, dtype)


def _closest(points, vertices, triangles, dtype, top=1, chunk=128):
    """the ``top`` smallest (d2, index) pairs per point, ascending -> d2 (N, top), tri (N, top), v, w; (+inf, -1) padding"""
    q_all = np.asarray(points, dtype=dtype)
    n, T = len(q_all), len(triangles)
    top = max(min(top, T), 1)
    d2 = np.full((n, top), np.inf, dtype=dtype)
    tri = np.full((n, top), -1, dtype=np.int64)
    bv, bw = np.zeros((n, top), dtype=dtype), np.zeros((n, top), dtype=dtype)
    if T == 0 or n == 0:
        return d2, tri, bv, bw
    v0, e1, e2, ok = _rows(vertices, triangles, dtype)
    for a in range(0, n, chunk):
        n2, v, w = tri_point(q_all[a:a + chunk, None, :], v0[None], e1[None], e2[None])
        n2 = np.where(ok[None] & ~np.isnan(n2), n2, np.inf)                # a NaN never wins
        order = np.argsort(n2, axis=1, kind="stable")[:, :top]             # the lowest index among equal d2
        got = np.take_along_axis(n2, order, axis=1)
        won = got < np.inf
        d2[a:a + chunk] = got
        tri[a:a + chunk] = np.where(won, order, -1)
        bv[a:a + chunk] = np.where(won, np.take_along_axis(v, order, axis=1), 0)
        bw[a:a + chunk] = np.where(won, np.take_along_axis(w, order, axis=1), 0)
    return d2, tri, bv, bw


def closest_oracle(points, vertices, triangles):
    """float64 -> {'d2', 'tri', 'v', 'w'} of the winner per point"""
    d2, tri, v, w = _closest(points, vertices, triangles, np.float64)
    return {"d2": d2[:, 0], "tri": tri[:, 0], "v": v[:, 0], "w": w[:, 0]}


def closest_fp32(points, vertices, triangles, top=1):
    """the kernels' formula in numpy float32 (inputs rounded to fp32 first)"""
    f = np.float32
    d2, tri, v, w = _closest(np.asarray(points, f), np.asarray(vertices, f), triangles, f, top=top)
    if top == 1:
        return {"d2": d2[:, 0], "tri": tri[:, 0], "v": v[:, 0], "w": w[:, 0]}
    return {"d2": d2, "tri": tri, "v": v, "w": w}


def pair_d2_oracle(points, vertices, triangles, tri):
    """float64 d2 from points[i] to triangle tri[i] (inf for tri[i] < 0)"""
    v0, e1, e2, _ = _rows(vertices, triangles, np.float64)
    t = np.maximum(np.asarray(tri), 0)
    if len(triangles) == 0:
        return np.full(len(points), np.inf)
    n2, _, _ = tri_point(np.asarray(points, np.float64), v0[t], e1[t], e2[t])
    return np.where(np.asarray(tri) >= 0, n2, np.inf)


def count_hits(origins, dirs, vertices, triangles, t_min=0.0, t_max=np.inf, dtype=np.float64):
    """the number of triangles that pass the hit test, all triangles, in ``dtype``"""
    n = len(origins)
    out = np.zeros(n, dtype=np.int32)
    if len(triangles) == 0 or n == 0:
        return out
    dt = dtype
    for sl, t, u, w, det, inside, _ in mc._all_triangles(np.asarray(origins, dt), np.asarray(dirs, dt), np.asarray(vertices, dt),
                                                         triangles, dt):
        with np.errstate(all="ignore"):
            out[sl] = (inside & (t >= dt(t_min)) & (t <= dt(t_max))).sum(axis=1)
    return out


def parity_rays(points):
    """the 3 N rays of contains(): ray j of point i at row j N + i"""
    p = np.asarray(points)
    return np.tile(p, (3, 1)), np.repeat(PARITY_DIRS, len(p), axis=0).astype(p.dtype)


def contains_oracle(points, vertices, triangles):
    """float64 parity vote -> (inside (N,) bool, counts (3, N), kept (N,) bool)"""
    p = np.asarray(points, np.float64)
    o, d = parity_rays(p)
    d32 = d.astype(np.float32).astype(np.float64)                         # the directions as the device sees them
    fin = np.isfinite(o).all(axis=1)
    o_f = np.where(fin[:, None], o, 0.0)
    counts = np.where(fin, count_hits(o_f, d32, vertices, triangles), 0).reshape(3, len(p))
    kept = mc.kept_rays(o_f, d32, vertices, triangles, np.full(len(o), np.inf)).reshape(3, len(p)).all(axis=0)
    return (counts & 1).sum(axis=0) >= 2, counts, kept


# ---- the lists of the build, restated ------------------------------------------------------------------------------------------
class Lists:
    """which cells of ``plan`` list a triangle, every operation in numpy float32 as mesh_bin_kernel orders them"""

    def __init__(self, vertices, triangles, plan, widen=True):
        f = np.float32
        self.plan = plan
        self.lo, self.cell = np.array(list(plan.bound_min), f), f(plan.cell)
        self.dims = np.array(list(plan.dims), np.int64)
        self.w, self.mag = f(plan.widen if widen else 0.0), f(plan.coord_mag)            # widen=False: lists without their slack w
        with np.errstate(all="ignore"):
            self.v0, self.e1, self.e2, self.ok = _rows(np.asarray(vertices, f), triangles, f)
            p1, p2 = self.v0 + self.e1, self.v0 + self.e2
            self.c_lo = self.cell_axis(np.minimum(self.v0, np.minimum(p1, p2)) - self.w)
            self.c_hi = self.cell_axis(np.maximum(self.v0, np.maximum(p1, p2)) + self.w)
            self.n = mc._cross(self.e1, self.e2)
            l1 = (np.abs(self.e1[:, 0]) + np.abs(self.e1[:, 1])) + np.abs(self.e1[:, 2])
            l2 = (np.abs(self.e2[:, 0]) + np.abs(self.e2[:, 1])) + np.abs(self.e2[:, 2])
            self.reach = (f(0.5) * self.cell + f(2.0) * self.w) * ((np.abs(self.n[:, 0]) + np.abs(self.n[:, 1])) + np.abs(self.n[:, 2])) * \
                (f(1.0) + f(2.0 ** -10)) + f(2.0 ** -20) * (l1 * l2) * ((l1 + l2) + f(2.0) * self.cell)

    def cell_axis(self, p):
        with np.errstate(all="ignore"):
            return np.clip(np.nan_to_num(np.floor((p - self.lo) / self.cell), nan=0.0), 0, (self.dims - 1).astype(np.float32)).astype(np.int64)

    def listed(self, tri, cells):
        """bool, broadcast over tri (...,) and cells (..., 3): the cell lists the triangle"""
        f = np.float32
        with np.errstate(all="ignore"):
            centre = self.lo + (cells.astype(f) + f(0.5)) * self.cell
            rel = centre - self.v0[tri]
            return self.ok[tri] & ((self.c_lo[tri] <= cells) & (cells <= self.c_hi[tri])).all(axis=-1) & \
                ~(np.abs(mc._dot(self.n[tri], rel)) > self.reach[tri])

    def cells_of(self, t):
        """(m, 3) int64: the cells that list triangle t"""
        if not self.ok[t]:
            return np.zeros((0, 3), np.int64)
        ax = [np.arange(self.c_lo[t, a], self.c_hi[t, a] + 1) for a in range(3)]
        cells = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
        return cells[self.listed(np.int64(t), cells)]


# ---- the shell walk of mesh_closest_kernel, restated -----------------------------------------------------------------------------
def _ring_finished(L, q, c, r, best, slack):
    """mesh_ring_finished (ring_gap + the stop test) in numpy fp32 for all queries at once; ``slack=False``: the bare rule"""
    f = np.float32
    with np.errstate(all="ignore"):
        g = np.full(len(q), np.inf, f)
        for a in range(3):
            lo_face = q[:, a] - (L.lo[a] + (c[:, a] - r).astype(f) * L.cell)
            hi_face = (L.lo[a] + (c[:, a] + r + 1).astype(f) * L.cell) - q[:, a]
            g = np.where(c[:, a] - r > 0, np.fmin(g, lo_face), g)
            g = np.where(c[:, a] + r < L.dims[a] - 1, np.fmin(g, hi_face), g)
        whole = g == np.inf
        if not slack:
            return whole | ((g > 0) & (best < g * g))
        gs = g - f(2.0 ** -18) * (L.mag + g)
        return whole | ((gs > 0) & (best < (gs * gs) * (f(1.0) - f(2.0 ** -20))))


def _first_ring(L, c, cand):
    """(N, K): the first shell of cell c[i] whose box holds a cell that lists candidate cand[i, k] (a huge number: none)"""
    out = np.full(cand.shape, np.iinfo(np.int64).max // 2, np.int64)
    for t in np.unique(cand[cand >= 0]):
        cells = L.cells_of(t)
        if not len(cells):
            continue
        i, k = np.nonzero(cand == t)
        for a in range(0, len(i), 512):                                   # (pairs, cells) at a time
            ii, kk = i[a:a + 512], k[a:a + 512]
            out[ii, kk] = np.abs(cells[None, :, :] - c[ii][:, None, :]).max(axis=2).min(axis=1)
    return out


def shells_fp32(vertices, triangles, points, plan, plan_far=None, rings=3, slack=True, max_candidates=32, top=None, widen=True):
    """The index route of miso_mesh_closest on the CPU: the lists, the Chebyshev shells around the query's clamped cell, the
    stop test after each, the restart on the coarse index after ``rings`` unfinished fine shells.  Per query the candidates
    are its ``max_candidates`` nearest triangles of the all-triangles pass in fp32; a candidate counts once a shell's box
    holds a cell that lists it (``top``: that pass, when the caller has it).  Queries must be finite and within 4 coord_mag
    (the others read all rows, by construction).  ``slack=False``: the bare stop test, best < g^2; ``widen=False``: lists
    built without their slack w (no index the library builds is like that).  -> (d2, tri, d2_all, tri_all, went_coarse)"""
    f = np.float32
    q = np.asarray(points, f)
    top = closest_fp32(q, vertices, triangles, top=max_candidates) if top is None else top
    tK, iK = top["d2"].reshape(len(q), -1), top["tri"].reshape(len(q), -1)
    n = len(q)
    best_d2, best_tri = np.full(n, np.inf, f), np.full(n, -1, np.int64)
    done = np.zeros(n, bool)
    coarse = np.zeros(n, bool)
    levels = [(Lists(vertices, triangles, plan, widen), rings if plan_far is not None else None)]
    if plan_far is not None:
        levels.append((Lists(vertices, triangles, plan_far, widen), None))
    found = np.zeros(tK.shape, bool)                                      # what the lane has seen stays seen
    for level, (L, r_end) in enumerate(levels):
        assert (np.isfinite(q).all(axis=1) & (np.abs(q) <= f(4.0) * L.mag).all(axis=1)).all(), "shells_fp32 restates the walk only"
        c = L.cell_axis(q)
        first = _first_ring(L, c, iK)
        if level == 1:
            coarse = ~done
        r_grid = int(L.dims.max())
        for r in range(r_grid if r_end is None else min(r_end, r_grid)):
            if done.all():
                break
            found |= (first <= r) & ~done[:, None] & (tK < np.inf)
            cur = np.where(found, tK, f(np.inf))
            k = np.argmin(cur, axis=1)                                    # candidates are sorted by (d2, index)
            rows = np.arange(n)
            b = cur[rows, k]
            fin = _ring_finished(L, q, c, r, b, slack) & ~done
            best_d2 = np.where(fin, b, best_d2)
            best_tri = np.where(fin, np.where(b < np.inf, iK[rows, k], -1), best_tri)
            done |= fin
    assert done.all(), "a walk ends at the latest when its box is the grid"
    return best_d2, best_tri, tK[:, 0], iK[:, 0], coarse


# ---- the counting walk (mesh_walk_ray with RayCount), restated -----------------------------------------------------------------------
def count_walk_fp32(vertices, triangles, origins, dirs, plan, t_min=0.0, t_max=np.inf, half_open=True):
    """The grid route of miso_mesh_count_hits on the CPU in numpy float32: clip, start cell, the DDA's boundaries from the
    cell index, and per visited cell the listed triangles whose computed t lies in the cell's stretch [t_in, t_out) -- the
    first stretch open below, the last open above, the boundaries a running maximum.  ``half_open=False`` counts a hit in
    every visited cell that lists it (what the rule is for).  -> (count, count_all): the walk's and the all-triangles count."""
    f = np.float32
    L = Lists(vertices, triangles, plan)
    lo, cell, dims, w = L.lo, L.cell, L.dims, L.w
    tri = np.asarray(triangles)
    o, d = np.asarray(origins, f), np.asarray(dirs, f)
    R = len(o)
    inf = f(np.inf)
    with np.errstate(all="ignore"):
        hits = []
        for sl, t, u, q, det, inside, _ in mc._all_triangles(o, d, np.asarray(vertices, f), tri, f):
            hits.append(np.where(inside & (t >= f(t_min)) & (t <= f(t_max)), t, inf))
        tt = np.concatenate(hits)
        count_all = (tt < inf).sum(axis=1).astype(np.int32)
        K = max(int(count_all.max()), 1)
        order = np.argsort(tt, axis=1, kind="stable")[:, :K]
        tK, iK = np.take_along_axis(tt, order, axis=1), order
        inv = np.where(d != 0, f(1.0) / d, f(0.0)).astype(f)
        step = np.sign(d).astype(np.int64)
        lo_w, hi_w = lo - w, (lo + dims.astype(f) * cell) + w
        ta, tb = (lo_w - o) * inv, (hi_w - o) * inv
        nz = d != 0
        t0 = np.maximum(f(t_min), np.where(nz, np.minimum(ta, tb), -inf).max(axis=1)).astype(f)
        t1 = np.minimum(f(t_max), np.where(nz, np.maximum(ta, tb), inf).min(axis=1)).astype(f)
        covered = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (np.abs(o) <= f(4.0) * L.mag).all(axis=1)
        assert covered.all(), "count_walk_fp32 restates the walk only (a ray outside its guarantee reads all rows)"
        miss = (~nz & ((o < lo_w) | (o > hi_w))).any(axis=1) | ~nz.any(axis=1)
        active = ~miss & (t0 <= t1)
        c = L.cell_axis(o + t0[:, None] * d)
        count = np.zeros(R, np.int32)
        t_in = np.full(R, -inf, f)
        rows = np.arange(R)
        for _ in range(int(dims.sum()) + 3):
            if not active.any():
                break
            ahead = (c + (step > 0)).astype(f)
            tm = np.where(step == 0, inf, ((lo + ahead * cell) - o) * inv).astype(f)
            t_out = tm.min(axis=1)
            ax = np.argmax(tm == t_out[:, None], axis=1)
            nxt = c[rows, ax] + step[rows, ax]
            last = (t_out > t1) | ~(t_out < inf) | (nxt < 0) | (nxt >= dims[ax])
            t_end = np.where(last, inf, np.maximum(t_in, t_out)).astype(f)
            here = L.listed(iK, c[:, None, :]) & (tK < inf) & active[:, None]
            if half_open:
                here &= (tK >= t_in[:, None]) & (tK < t_end[:, None])
            count += here.sum(axis=1).astype(np.int32)
            active &= ~last
            c[rows[active], ax[active]] = nxt[active]
            t_in = t_end
    return count, count_all


# ---- fixtures ------------------------------------------------------------------------------------------------------------------
def _near_and_uniform(rng, vertices, triangles, n_near, n_uniform, sigma, inflate):
    """points near the surface (on a random hittable triangle, moved by a Gaussian) and uniform in the inflated box"""
    ok = mc.hittable(vertices, triangles)
    v = np.asarray(vertices, np.float64)[np.asarray(triangles)[ok]]
    pick = rng.integers(0, len(v), size=n_near)
    b = rng.dirichlet((1.0, 1.0, 1.0), size=n_near)
    near = (v[pick] * b[:, :, None]).sum(axis=1) + sigma * rng.standard_normal((n_near, 3))
    lo, hi = v.reshape(-1, 3).min(axis=0) - inflate, v.reshape(-1, 3).max(axis=0) + inflate
    return np.concatenate([near, rng.uniform(lo, hi, size=(n_uniform, 3))])


def _fixture(name, vertices, triangles, points, cells, closed):
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32))          # noqa: E731
    return {"name": name, "vertices": f32(vertices), "triangles": np.ascontiguousarray(triangles, dtype=np.int64),
            "points": f32(points), "cells": cells, "closed": closed}


def cube():
    """the box [0, 4]^3 (integer vertices) and the half-integer lattice of [-1.5, 5.5]^3: points on faces, edges, vertices,
    at the centre (every face ties: the lowest index wins), inside and outside; every value is exact in fp32"""
    v, t = mc.box((0, 0, 0), (4, 4, 4))
    g = np.arange(-1.5, 5.75, 0.5)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return _fixture("cube", v, t, p, (0.5, 1.0), True)


def _from_mesh_cases(name, seed, sigma, inflate, closed=False, n=2048):
    fx = mc.FIXTURES[name]()
    rng = np.random.default_rng(seed)
    p = _near_and_uniform(rng, fx["vertices"], fx["triangles"], n - n // 4, n // 4, sigma, inflate)
    return _fixture(name, fx["vertices"], fx["triangles"], p, fx["cells"], closed)


def far():
    """room's mesh; queries for each route: near the surface (the fine shells), a cloud about the room's centre (the coarse
    index), and a few finite points beyond 4 coord_mag (all rows)"""
    fx = mc.room()
    rng = np.random.default_rng(23)
    near = _near_and_uniform(rng, fx["vertices"], fx["triangles"], 512, 0, 0.01, 0.0)
    centre = np.array([4.0, 3.0, 1.6]) + 0.3 * rng.standard_normal((256, 3))
    beyond = np.array([[100.0, 3.0, 1.0], [4.0, -90.0, 1.0], [4.0, 3.0, 200.0], [-170.0, -170.0, -170.0], [4.0, 3.0, -150.0]])
    out = _fixture("far", fx["vertices"], fx["triangles"], np.concatenate([near, centre, beyond]), fx["cells"], False)
    out["n_beyond"] = len(beyond)
    return out


def nested():
    """a box inside a box: between the two is inside (one crossing), inside the inner box is outside again (two)"""
    v, t = mc.join([mc.box((-1.0, -1.0, -1.0), (3.0, 2.5, 2.0)), mc.box((0.0, 0.0, 0.0), (1.5, 1.0, 1.0))])
    rng = np.random.default_rng(29)
    p = np.concatenate([_near_and_uniform(rng, v, t, 512, 1024, 0.05, 0.5), rng.uniform((0, 0, 0), (1.5, 1, 1), size=(256, 3))])
    return _fixture("nested", v, t, p, (0.3, 0.9), True)


def nested_inside(points):
    """the parity answer of `nested`, analytically (points on a face excluded by the callers' kept mask)"""
    p = np.asarray(points, np.float64)
    outer = ((p > (-1.0, -1.0, -1.0)) & (p < (3.0, 2.5, 2.0))).all(axis=1)
    inner = ((p > (0.0, 0.0, 0.0)) & (p < (1.5, 1.0, 1.0))).all(axis=1)
    return outer & ~inner


def made_face_case(cell=0.37):
    """One query for which the bare stop test loses on lists built WITHOUT their slack w.  On straddle's grid (bounds
    from -75.14) some computed face fl(lo + fl(k cell)) lies a few ulps ABOVE points that membership
    floor(fl(fl(x - lo) / cell)) already puts in cell k.  Triangle 0 lies in such a plane x = x_t, in cell k; the query
    sits 0.1 below it in cell k - 1, and triangle 1 lies in the query's cell on the other side, farther than triangle 0
    by less than the face's error: after shell 0 the bare test sees triangle 1 inside the computed gap and stops.
    -> a fixture dict with one point; the answer is triangle 0."""
    f = np.float32
    lo, c = f(-75.14), f(cell)
    best = None
    for k in range(2, 400):
        face = f(lo + f(f(k) * c))
        x = face
        for j in range(1, 5):
            x = np.nextafter(x, f(-np.inf))
            if np.floor(f(f(x - lo) / c)) >= k and (best is None or j > best[0]):
                best = (j, k, x, face)
    j, k, x_t, face = best
    q = np.array([float(x_t) - 0.1, float(lo) + 203.5 * cell, 4.5 * cell])        # y and z: a cell's centre, 0.185 from its faces
    gap = float(face) - float(x_t)                                        # j ulps of the coordinate, about 1e-5
    x_b = q[0] - (0.1 + 0.5 * gap)

    def tri_in_plane(x):
        return np.array([[x, q[1] - 0.5, q[2] - 0.5], [x, q[1] + 0.5, q[2] - 0.5], [x, q[1], q[2] + 0.5]])

    corners = np.array([[-75.14, -75.14, 0.0], [-75.14, -75.0, 0.0], [-75.0, -75.14, 0.1], [75.0, 75.0, 3.0], [75.0, 74.9, 3.0], [74.9, 75.0, 2.9]])
    v = np.concatenate([tri_in_plane(float(x_t)), tri_in_plane(x_b), corners])
    out = _fixture("made_face", v, np.arange(len(v), dtype=np.int64).reshape(-1, 3), q[None], (cell, 7.9), False)
    out["k"], out["ulps"] = k, j
    return out


FIXTURES = {"cube": cube,
            "room": lambda: _from_mesh_cases("room", 31, 0.1, 0.5, closed=False),
            "open": lambda: _from_mesh_cases("open", 37, 0.1, 0.5),
            "sliver": lambda: _from_mesh_cases("sliver", 41, 0.1, 0.5),
            "straddle": lambda: _from_mesh_cases("straddle", 43, 0.2, 0.5),
            "far": far, "nested": nested}
CLOSED = ("cube", "nested")                # the fixtures whose surface is closed: parity means inside


@functools.lru_cache(maxsize=None)
def fixture(name):
    """the fixture with its oracle: adds 'ref' (float64 over the fp32 inputs as the device sees them) and 'coord_max'"""
    fx = dict(FIXTURES[name]())
    fx["ref"] = closest_oracle(fx["points"], fx["vertices"], fx["triangles"])
    ok = mc.hittable(fx["vertices"], fx["triangles"])
    used = fx["vertices"][fx["triangles"][ok]].astype(np.float64)
    fx["walks"] = np.isfinite(fx["points"]).all(axis=1)
    if "n_beyond" in fx:
        fx["walks"][len(fx["points"]) - fx["n_beyond"]:] = False
    fx["coord_max"] = float(max(np.abs(used).max(), np.abs(fx["points"][np.isfinite(fx["points"]).all(axis=1)]).max()))
    return fx


@functools.lru_cache(maxsize=None)
def candidates(name, k=32):
    """the k nearest triangles in fp32 of the fixture's walking queries: shells_fp32's ``top``"""
    fx = fixture(name)
    return closest_fp32(fx["points"][fx["walks"]], fx["vertices"], fx["triangles"], top=k)


@functools.lru_cache(maxsize=None)
def parity(name):
    """float64 parity of the fixture's points: (inside, counts (3, N), kept)"""
    fx = fixture(name)
    return contains_oracle(fx["points"], fx["vertices"], fx["triangles"])


@functools.lru_cache(maxsize=None)
def lattice():
    """mesh_cases' lattice with its {0, +-1}^3 rays and the float64 crossing counts: exact in fp32, every ray kept"""
    fx = dict(mc.lattice())
    fx["count"] = count_hits(fx["origins"], fx["dirs"], fx["vertices"], fx["triangles"])
    return fx


def d_error(fx, d2, tri=None):
    """e of the module docstring per query with a finite float64 answer (nan elsewhere); with ``tri`` also the float64
    distance of the triangle the caller chose, as an error against the best: (e, e_tri)"""
    ref = np.sqrt(fx["ref"]["d2"])
    with np.errstate(all="ignore"):
        e = np.where(np.isfinite(ref), np.abs(np.sqrt(np.asarray(d2, np.float64)) - ref) / (fx["coord_max"] + ref), np.nan)
        if tri is None:
            return e
        own = np.sqrt(pair_d2_oracle(fx["points"], fx["vertices"], fx["triangles"], tri))
        return e, np.where(np.isfinite(ref), (own - ref) / (fx["coord_max"] + ref), np.nan)


def measure_fp32_error():
    """max e over all fixtures under closest_fp32: the figure behind FP32_E_MAX"""
    worst = {}
    for name in FIXTURES:
        fx = fixture(name)
        e = d_error(fx, closest_fp32(fx["points"], fx["vertices"], fx["triangles"])["d2"])
        worst[name] = float(np.nanmax(e)) if np.isfinite(e).any() else 0.0
    return max(worst.values()), worst
