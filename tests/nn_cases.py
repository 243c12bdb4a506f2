"""Seeded clouds for the nearest-neighbour tests (tests/test_nearest.py, tests/test_mesh_eval.py), a float64 all-pairs
search, and a float64 restatement of the cell-list query's ring rule (csrc/nn.hip) that the CPU tests run on the fixtures
themselves.  Nothing here touches the library; every cloud is generated, none is stored."""
import functools

import numpy as np

F32 = np.float32


# --------------------------------------------------------------------------- float64 references
def all_pairs64(src, tgt, chunk=512):
    """For every row of src (N,3) the smallest true squared distance to a row of tgt (M,3) and the LOWEST index that
    attains it, in float64 on the given (fp32) values, exactly converted.  Rows with a non-finite coordinate match
    nothing: (inf, -1) for a query without a match."""
    s, t = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(tgt, dtype=np.float64).reshape(-1, 3)
    n, m = len(s), len(t)
    D, I = np.full(n, np.inf), np.full(n, -1, dtype=np.int64)
    if m == 0 or n == 0:
        return D, I
    for a in range(0, n, chunk):
        with np.errstate(invalid="ignore", over="ignore"):
            diff = s[a:a + chunk, None, :] - t[None, :, :]
            d2 = ((diff[..., 0] ** 2 + diff[..., 1] ** 2) + diff[..., 2] ** 2)
        d2 = np.where(np.isfinite(d2), d2, np.inf)
        j = np.argmin(d2, axis=1)                      # the first minimum: the lowest index
        best = d2[np.arange(len(j)), j]
        D[a:a + chunk] = best
        I[a:a + chunk] = np.where(np.isfinite(best), j, -1)
    return D, I


def true_d2(src, tgt, idx):
    """float64 squared distance of query i to target idx[i] (inf where idx < 0)"""
    s, t = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(tgt, dtype=np.float64).reshape(-1, 3)
    idx = np.asarray(idx)
    out = np.full(len(s), np.inf)
    ok = idx >= 0
    with np.errstate(invalid="ignore", over="ignore"):
        d = s[ok] - t[idx[ok]]
        out[ok] = (d[:, 0] ** 2 + d[:, 1] ** 2) + d[:, 2] ** 2
    return out


def plan64(tgt, cell, cap=1 << 24):
    """bound_min, dims and the cell used, as miso_nn_plan forms them (bounds of the finite rows)"""
    t = np.asarray(tgt, dtype=np.float64).reshape(-1, 3)
    t = t[np.isfinite(t).all(axis=1)]
    lo, hi = (t.min(axis=0), t.max(axis=0)) if len(t) else (np.zeros(3), np.zeros(3))
    lo32, ext = lo.astype(F32), (hi.astype(F32) - lo.astype(F32)).astype(F32)     # the kernels' fp32 difference and division
    c = F32(cell)
    while np.prod(np.floor(ext / c).astype(np.float64) + 1.0) > cap:
        c = F32(c * F32(2.0))
    return lo, hi, (np.floor(ext / c).astype(np.int64) + 1), float(c)


def ring_rule64(src, tgt, cell, max_rings):
    """The query of csrc/nn.hip in float64, all candidates compared at once: after ring r the examined box is the
    cells within Chebyshev distance r of the query's (clamped) cell, and the query is finished when its best distance
    is <= g, the smallest distance to a face of that box that is not on the grid's edge (or when every face is).
    -> (rings, idx): rings[i] = the first ring after which query i is finished (max_rings + 1 = not finished by then), idx
    its answer then (-1 where unfinished).  Finite rows only."""
    s, t = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(tgt, dtype=np.float64).reshape(-1, 3)
    lo, _, dims, c = plan64(t, cell)
    tc = np.clip(np.floor((t - lo) / c), 0, dims - 1).astype(np.int64)
    qc = np.clip(np.floor((s - lo) / c), 0, dims - 1).astype(np.int64)
    rings = np.full(len(s), max_rings + 1, dtype=np.int64)
    idx = np.full(len(s), -1, dtype=np.int64)
    for a in range(0, len(s), 256):
        q, c0 = s[a:a + 256], qc[a:a + 256]
        diff = q[:, None, :] - t[None, :, :]
        d2 = (diff[..., 0] ** 2 + diff[..., 1] ** 2) + diff[..., 2] ** 2
        cheb = np.abs(c0[:, None, :] - tc[None, :, :]).max(axis=2)
        open_ = np.ones(len(q), dtype=bool)
        for r in range(max_rings + 1):
            seen = np.where(cheb <= r, d2, np.inf)
            j = np.argmin(seen, axis=1)
            best = np.sqrt(seen[np.arange(len(q)), j])
            g = np.full(len(q), np.inf)
            for ax in range(3):
                low, high = c0[:, ax] - r, c0[:, ax] + r
                g = np.where(low > 0, np.minimum(g, q[:, ax] - (lo[ax] + low * c)), g)
                g = np.where(high < dims[ax] - 1, np.minimum(g, (lo[ax] + (high + 1) * c) - q[:, ax]), g)
            fin = open_ & (best <= g)
            rings[a:a + 256][fin] = r
            idx[a:a + 256][fin] = np.where(np.isfinite(best[fin]), j[fin], -1)
            open_ &= ~fin
    return rings, idx


# --------------------------------------------------------------------------- clouds
def box_surface(rng, n, size, origin=(0.0, 0.0, 0.0)):
    """n points uniform (by area) on the six faces of the box [origin, origin + size]"""
    sx, sy, sz = size
    areas = np.array([sy * sz, sy * sz, sx * sz, sx * sz, sx * sy, sx * sy])
    face = rng.choice(6, size=n, p=areas / areas.sum())
    p = rng.random((n, 3)) * np.asarray(size)
    axis, side = face // 2, face % 2
    p[np.arange(n), axis] = side * np.asarray(size)[axis]
    return p + np.asarray(origin)


def _room():
    rng = np.random.default_rng(1201)
    size = (4.0, 3.0, 2.5)
    tgt = box_surface(rng, 3001, size)
    src = box_surface(rng, 2053, size) + rng.normal(0.0, 0.01, (2053, 3))
    d = rng.normal(size=(103, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    src[:103] = 0.5 * np.asarray(size) + d * rng.uniform(4.0, 7.0, (103, 1))
    return dict(tgt=tgt, src=src, cell=0.1, max_rings=4)


def _far():
    rng = np.random.default_rng(1202)
    tgt = box_surface(rng, 1500, (1.0, 1.0, 1.0))
    src = box_surface(rng, 700, (1.0, 1.0, 1.0)) + 3.0 / np.sqrt(3.0)
    return dict(tgt=tgt, src=src, cell=0.05, max_rings=4)


def _lattice():
    k = np.arange(9) / 8.0
    tgt = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
    c = (np.arange(8) + 0.5) / 8.0
    src = np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1).reshape(-1, 3)
    return dict(tgt=tgt, src=src, cell=0.125, max_rings=4)


def _step(x, ulps):
    x = F32(x)
    for _ in range(abs(ulps)):
        x = np.nextafter(x, F32(np.inf if ulps > 0 else -np.inf), dtype=F32)
    return x


def _faces():
    """Around 37 m an fp32 ulp is 3.8e-6.  Per (face k, offset j): target A j ulps from the face min + k cell of the x axis,
    the query 1 mm above the face, target B in the query's cell two ulps farther from it than A.  A is the nearest; a
    stop test without rounding slack can finish on B when A's cell (by the fp32 floor) is the one below."""
    origin = np.array([F32(37.03), F32(36.91), F32(37.17)], dtype=F32)
    cell = F32(0.1)
    tgt, src = [origin.copy(), (origin + np.array([3.0, 2.5, 2.5], dtype=F32)).astype(F32)], []
    g = 0
    for k in range(1, 29):
        for j in range(-4, 5):
            y = F32(origin[1] + F32(0.13) * F32(1 + g % 16))
            z = F32(origin[2] + F32(0.13) * F32(1 + g // 16))
            g += 1
            face = F32(origin[0] + F32(k) * cell)
            ax = _step(face, j)
            qx = F32(face + F32(0.001))
            bx = _step(F32(qx + F32(qx - ax)), 2)
            tgt += [np.array([ax, y, z], dtype=F32), np.array([bx, y, z], dtype=F32)]
            src.append(np.array([qx, y, z], dtype=F32))
    return dict(tgt=np.stack(tgt), src=np.stack(src), cell=0.1, max_rings=4)


def cell32(x, lo, cell, dim=None):
    """the kernels' cell index along one axis in their own arithmetic: floor(fl(fl(x - lo) / cell)), clamped"""
    c = np.floor((F32(x) - F32(lo)).astype(F32) / F32(cell))
    return np.clip(c, 0, None if dim is None else dim - 1).astype(np.int64)


def _straddle():
    """Bounds that span zero with an extent comparable to |lo|: t - lo is then inexact (its ulp is many ulps of t), so a
    target up to ~16 ulps ABOVE the computed face fl(lo + fl(k cell)) is still binned in the cell below.  Per face k:
    A = the highest such coordinate, the query 0.2 mm above the computed face (in cell k), B in the query's cell at a
    distance half way between d_A and g = fl(q - face).  A is the nearest; a stop test without rounding slack sees
    best = d_B <= g after ring 0 and answers B, off by 1e-3 .. 5e-2 in d (tests/test_nearest.py checks that it does)."""
    lo = np.array([F32(-75.14), F32(-1.0), F32(-1.0)], dtype=F32)
    hi = np.array([F32(75.0), F32(1.0), F32(1.0)], dtype=F32)
    cell = F32(0.0475)
    tgt, src, groups = [lo.copy(), hi.copy()], [], []
    g = 0
    for k in range(600, 3000, 7):
        face = F32(lo[0] + F32(F32(k) * cell))
        ax = None
        x = face
        for _ in range(64):                                   # the highest coordinate above the face still binned below it
            x = np.nextafter(x, F32(np.inf), dtype=F32)
            if cell32(x, lo[0], cell) == k - 1:
                ax = x
        qx = F32(face + F32(0.0002))
        if ax is None or cell32(qx, lo[0], cell) != k or not ax < qx:
            continue
        gc = F32(qx - face)
        da = float(qx) - float(ax)
        bx = F32(float(qx) + 0.5 * (da + float(gc)))
        if not (da < float(bx) - float(qx) <= float(gc)) or cell32(bx, lo[0], cell) != k:
            continue
        if g == 100:
            break
        y = F32(-0.9 + 0.2 * (g % 10))
        z = F32(-0.9 + 0.2 * (g // 10))
        g += 1
        groups.append((len(src), len(tgt), len(tgt) + 1))      # (query, A, B)
        tgt += [np.array([ax, y, z], dtype=F32), np.array([bx, y, z], dtype=F32)]
        src.append(np.array([qx, y, z], dtype=F32))
    return dict(tgt=np.stack(tgt), src=np.stack(src), cell=float(cell), max_rings=4, groups=np.asarray(groups))


def ring0_fp32(c, slack):
    """Ring 0 of the kernel's query in its own fp32 arithmetic for every query of case `c`: the best target of the
    query's cell and the stop test after it, with the rounding slack of csrc/nn.hip (ring_finished) or, slack=False, the
    bare rule best <= g.  -> (finished (N,) bool, idx (N,))"""
    t, s = c["tgt"], c["src"]
    lo, _, dims, cell = plan64(t, c["cell"])
    lo, cell = lo.astype(F32), F32(cell)
    ext = [float(dims[a]) * float(cell) for a in range(3)]
    mag = F32(max(max(abs(float(lo[a])), abs(float(lo[a]) + ext[a])) + ext[a] for a in range(3)) * (1.0 + 1e-6))
    tc = np.stack([cell32(t[:, a], lo[a], cell, dims[a]) for a in range(3)], axis=1)
    qc = np.stack([cell32(s[:, a], lo[a], cell, dims[a]) for a in range(3)], axis=1)
    fin, idx = np.zeros(len(s), dtype=bool), np.full(len(s), -1, dtype=np.int64)
    for i in range(len(s)):
        own = np.nonzero((tc == qc[i]).all(axis=1))[0]
        best = F32(np.inf)
        if len(own):
            d = (s[i] - t[own]).astype(F32)
            d2 = ((d[:, 0] * d[:, 0]).astype(F32) + (d[:, 1] * d[:, 1]).astype(F32)).astype(F32)
            d2 = (d2 + (d[:, 2] * d[:, 2]).astype(F32)).astype(F32)
            j = int(np.argmin(d2))
            best, idx[i] = d2[j], own[j]
        g = F32(np.inf)
        for a in range(3):
            if qc[i, a] > 0:
                g = min(g, F32(s[i, a] - F32(lo[a] + F32(F32(qc[i, a]) * cell))))
            if qc[i, a] < dims[a] - 1:
                g = min(g, F32(F32(lo[a] + F32(F32(qc[i, a] + 1) * cell)) - s[i, a]))
        if not slack:
            fin[i] = np.isinf(g) or (g > 0 and best <= F32(g * g))
        else:
            gs = F32(g - F32(F32(2.0 ** -21) * F32(mag + g)))
            fin[i] = np.isinf(g) or (gs > 0 and best < F32(F32(gs * gs) * F32(1.0 - 2.0 ** -20)))
    return fin, idx


def _crowd():
    rng = np.random.default_rng(1205)
    centre = np.array([0.31, 0.62, 0.43])
    tgt = np.concatenate([centre + rng.uniform(-0.001, 0.001, (2000, 3)), rng.random((500, 3))])
    src = np.concatenate([rng.random((300, 3)), centre + rng.uniform(-0.01, 0.01, (100, 3))])
    return dict(tgt=tgt[rng.permutation(len(tgt))], src=src, cell=0.05, max_rings=4)


def _capped():
    rng = np.random.default_rng(1206)
    tgt = np.concatenate([rng.random((800, 3)), 999.0 + rng.random((800, 3))])
    src = np.concatenate([rng.random((200, 3)) * 1.5, 998.5 + rng.random((200, 3)) * 1.5])
    return dict(tgt=tgt, src=src, cell=0.05, max_rings=4)


def _dup():
    rng = np.random.default_rng(1207)
    t = rng.random((600, 3))
    return dict(tgt=np.concatenate([t, t]), src=rng.random((500, 3)), cell=0.08, max_rings=4)


def _nan():
    rng = np.random.default_rng(1208)
    tgt, src = rng.random((400, 3)), rng.random((300, 3))
    tgt[[3, 77], 0] = np.nan
    tgt[150, 2] = np.inf
    tgt[151, 1] = -np.inf
    src[[0, 41], 1] = np.nan
    src[100, 0] = np.inf
    src[299, 2] = -np.inf
    return dict(tgt=tgt, src=src, cell=0.1, max_rings=4)


def _sized(n, seed):
    def make():
        rng = np.random.default_rng(seed)
        return dict(tgt=rng.random((1031, 3)), src=rng.random((n, 3)), cell=0.1, max_rings=4)
    return make


def _small(m, n, seed):
    def make():
        rng = np.random.default_rng(seed)
        return dict(tgt=rng.random((m, 3)), src=rng.random((n, 3)), cell=0.1, max_rings=4)
    return make


def _segments():
    """Seventeen LDS tiles of 1024 targets, the last one partial, for the all-pairs kernel behind the rings: two rings at
    0.05 leave the shifted queries to it."""
    rng = np.random.default_rng(1216)
    tgt = box_surface(rng, 17161, (1.0, 1.0, 1.0))
    src = np.concatenate([box_surface(rng, 230, (1.0, 1.0, 1.0)) + 0.7, rng.random((100, 3))])
    return dict(tgt=tgt, src=src, cell=0.05, max_rings=2)


def _all_nan_targets():
    rng = np.random.default_rng(1215)
    return dict(tgt=np.full((37, 3), np.nan), src=rng.random((70, 3)), cell=0.1, max_rings=4)


_MAKERS = {"room": _room, "far": _far, "lattice": _lattice, "faces": _faces, "crowd": _crowd, "capped": _capped,
           "dup": _dup, "single": _small(1, 130, 1209), "one_query": _small(257, 1, 1210), "empty": _small(0, 70, 1211),
           "straddle": _straddle, "nan": _nan, "nan_targets": _all_nan_targets, "segments": _segments, **{f"n{n}": _sized(n, 1300 + n) for n in (63, 64, 65, 255, 257)}}
NAMES = tuple(_MAKERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(tgt (M,3) fp32, src (N,3) fp32, cell, max_rings), read-only and shared"""
    c = _MAKERS[name]()
    for k in ("tgt", "src"):
        c[k] = np.ascontiguousarray(c[k], dtype=F32).reshape(-1, 3)
        c[k].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (D* (N,) float64, lowest index that attains it (N,)), computed once per case"""
    c = case(name)
    D, I = all_pairs64(c["src"], c["tgt"])
    D.setflags(write=False)
    I.setflags(write=False)
    return D, I


# --------------------------------------------------------------------------- meshes
def icosphere(radius=1.0, subdivisions=4):
    """A subdivided icosahedron: 20 * 4^subdivisions faces (5120 at 4), vertices on the sphere of ``radius``."""
    p = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
         (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    v = [np.asarray(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v) * radius, np.asarray(f, dtype=np.int64)
