"""Seeded clouds for the ICP tests (tests/test_icp_host.py, tests/test_icp.py) and float64 numpy restatements of what
csrc/icp.hip and grid_opt/utils/utils_registration.py compute: ``transform64``, ``sums64``, ``normals64``, ``icp_loop64``.
Nothing here touches the library; every cloud is generated, none is stored.

The shape has no symmetry, so a pose is observable: the surface of a 4 x 3 x 2.5 box (the room) plus a 1 x 0.6 x 0.8 box
standing off-centre on its floor."""
import functools
import math

import numpy as np

import nn_cases as nc

F32 = np.float32
ROOM = (4.0, 3.0, 2.5)
BLOCK, BLOCK_AT = (1.0, 0.6, 0.8), (0.7, 1.9, 0.0)
SUMS = 32

# max_dist of the sums fixture (a 3 deg / 5 cm offset leaves roughly half of the pairs beyond it), Tukey's k there, the
# radius of the normals fixture (four point spacings of 6 000 points on 63 m^2), and the demo's two thresholds
SUMS_MAX_DIST, SUMS_TUKEY_K, NORMALS_RADIUS = 0.08, 0.03, 0.4
COARSE, FINE, TUKEY_K = 0.02 * 15, 0.02 * 1.5, 1e-2

# Independent samplings (tests/test_icp.py, case 6): what icp_loop64 reaches on the CPU for fixture(),
# coarse then fine, measured once with tests/test_icp_host.py::test_icp_loop64_on_independent_samplings (which asserts
# that the loop still reaches it).  (translation error in metres, rotation error in radians) per kind.
INDEPENDENT_REACHED = {"point_to_plane": (5.43e-5, 1.91e-5), "point_to_point": (2.77e-3, 1.23e-3)}


# --------------------------------------------------------------------------- poses
def pose(deg, metres, axis=(1.0, 2.0, 3.0), direction=(2.0, -1.0, 1.0)):
    """4 x 4 float64: a rotation of ``deg`` degrees about ``axis`` and a translation of length ``metres``"""
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = math.radians(deg)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)
    T[:3, 3] = np.asarray(direction, dtype=np.float64) / np.linalg.norm(direction) * metres
    return T


def pose_error(T, want):
    """(translation error, rotation angle) of T against ``want``"""
    E = (np.linalg.inv(want) @ T)[:3, :3]
    sine = np.linalg.norm(0.5 * (E - E.T)) / math.sqrt(2.0)          # |sin(angle)|: no cancellation at small angles
    return float(np.linalg.norm(T[:3, 3] - want[:3, 3])), float(np.arcsin(min(sine, 1.0)))


def apply64(T, p):
    p = np.asarray(p, dtype=np.float64)
    return p @ T[:3, :3].T + T[:3, 3]


# --------------------------------------------------------------------------- the shape
def shape_surface(rng, n):
    """n points uniform by area on the room and the block -> (points (n, 3) float64, unit face normals (n, 3))"""
    def box(count, size, origin):
        p = nc.box_surface(rng, count, size)
        s = np.asarray(size)
        on = (p == 0.0) | (p == s)                                     # the face coordinate was assigned, not drawn
        axis = np.argmax(on, axis=1)
        nrm = np.zeros((count, 3))
        nrm[np.arange(count), axis] = np.where(p[np.arange(count), axis] == 0.0, -1.0, 1.0)
        return p + np.asarray(origin), nrm

    area = lambda s: 2.0 * (s[0] * s[1] + s[1] * s[2] + s[2] * s[0])    # noqa: E731
    n_block = int(round(n * area(BLOCK) / (area(ROOM) + area(BLOCK))))
    a, an = box(n - n_block, ROOM, (0.0, 0.0, 0.0))
    b, bn = box(n_block, BLOCK, BLOCK_AT)
    order = rng.permutation(n)
    return np.concatenate([a, b])[order], np.concatenate([an, bn])[order]


def shape_mesh(cells=8):
    """The same shape as a triangle mesh (vertices (V, 3) float64, faces (F, 3)): every box face a grid of
    ``cells`` x ``cells`` quads, two triangles each, outward winding."""
    verts, faces = [], []
    for size, origin in ((ROOM, (0.0, 0.0, 0.0)), (BLOCK, BLOCK_AT)):
        for axis in range(3):
            u, v = (axis + 1) % 3, (axis + 2) % 3
            for side in (0, 1):
                k = np.arange(cells + 1) / cells
                g = np.zeros((cells + 1, cells + 1, 3))
                g[..., u], g[..., v], g[..., axis] = k[:, None] * size[u], k[None, :] * size[v], side * size[axis]
                base = sum(len(x) for x in verts)
                verts.append(g.reshape(-1, 3) + np.asarray(origin))
                i, j = np.meshgrid(np.arange(cells), np.arange(cells), indexing="ij")
                a = base + (i * (cells + 1) + j).ravel()
                b, c, d = a + (cells + 1), a + (cells + 1) + 1, a + 1
                tri = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
                faces.append(tri if side else tri[:, ::-1])
    return np.concatenate(verts), np.concatenate(faces).astype(np.int64)


# --------------------------------------------------------------------------- float64 restatements
def transform64(T, p):
    """R p + t in float64 for the pose the kernel receives (T rounded to fp32) -> (p' (N, 3), bound (N, 3)) with
    bound_i = sum_j |R_ij| |p_j| + |t_i|, the magnitude miso_icp_transform's rounding error scales with"""
    T32 = np.asarray(T, dtype=np.float64).astype(F32).astype(np.float64)
    p = np.asarray(p, dtype=np.float64)
    return p @ T32[:3, :3].T + T32[:3, 3], np.abs(p) @ np.abs(T32[:3, :3]).T + np.abs(T32[:3, 3])


def _fsum_columns(terms):
    return np.array([math.fsum(terms[:, a]) for a in range(terms.shape[1])]) if len(terms) else np.zeros(terms.shape[1])


def sums64(moved, d2, idx, tgt, normals=None, max_dist=0.0, kind="point_to_plane", tukey_k=None, origin=(0.0, 0.0, 0.0)):
    """The block of sums of miso_icp_sums: every term in float64 in the kernel's order of operations (csrc/icp.hip), the
    columns added exactly (math.fsum).  -> (sums (32,), sums of |terms| (32,), inlier mask)"""
    p, dd = np.asarray(moved, dtype=np.float64).reshape(-1, 3), np.asarray(d2, dtype=np.float64).reshape(-1)
    idx, t = np.asarray(idx, dtype=np.int64).reshape(-1), np.asarray(tgt, dtype=np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        inl = (idx >= 0) & (idx < len(t)) & (dd <= max_dist * max_dist)
    p, dd, q = p[inl], dd[inl], t[idx[inl]]
    terms = np.zeros((len(p), SUMS))
    terms[:, 0], terms[:, 1] = 1.0, dd
    if kind == "point_to_plane":
        n = np.asarray(normals, dtype=np.float64).reshape(-1, 3)[idx[inl]]
        e = p - q
        r = (e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2]
        J = np.stack([p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2],
                      p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]], axis=1)
        w = np.ones(len(p))
        if tukey_k is not None:
            s = r / tukey_k
            u = 1.0 - s * s
            w = np.where(np.abs(r) <= tukey_k, u * u, 0.0)
        at = 2
        for a in range(6):
            wj = w * J[:, a]
            for b in range(a, 6):
                terms[:, at] = wj * J[:, b]
                at += 1
        for a in range(6):
            terms[:, 23 + a] = (w * J[:, a]) * r
        terms[:, 29] = (w * r) * r
    else:
        o = np.asarray(origin, dtype=np.float64)
        a3, b3 = p - o, q - o
        terms[:, 2:5], terms[:, 5:8] = a3, b3
        for a in range(3):
            for b in range(3):
                terms[:, 8 + 3 * a + b] = b3[:, a] * a3[:, b]
    return _fsum_columns(terms), _fsum_columns(np.abs(terms)), inl


def normals64(tgt, pts, radius, chunk=256):
    """For every row of pts: the targets with d2 <= radius^2 (d = t - q and d2 = (dx dx + dy dy) + dz dz in float64, the
    kernel's arithmetic), their count, numpy.linalg.eigh's eigenvector of the smallest eigenvalue of their (centred)
    covariance, and the eigen-gap (l1 - l0) / l2.  Fewer than three neighbours: (0, 0, 1), gap 0.
    -> (normals (N, 3), counts (N,), gaps (N,))"""
    t, q = np.asarray(tgt, dtype=np.float64).reshape(-1, 3), np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    normals, counts, gaps = np.tile([0.0, 0.0, 1.0], (len(q), 1)), np.zeros(len(q), dtype=np.int64), np.zeros(len(q))
    for a in range(0, len(q), chunk):
        d = t[None, :, :] - q[a:a + chunk, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        near = d2 <= radius * radius
        counts[a:a + chunk] = near.sum(axis=1)
        for i in np.nonzero(counts[a:a + chunk] >= 3)[0]:
            nb = d[i][near[i]]
            c = nb - nb.mean(axis=0)
            vals, vecs = np.linalg.eigh(c.T @ c / len(nb))
            normals[a + i] = vecs[:, 0]
            gaps[a + i] = (vals[1] - vals[0]) / vals[2] if vals[2] > 0 else 0.0
    return normals, counts, gaps


def nearest64(src, tgt):
    """nn_cases.all_pairs64's answer (the true nearest in float64, the lowest index on a tie) at the cost of a matrix
    product: |s|^2 + |t|^2 - 2 s.t, whose error here is below 1e-12, picks the candidates within 1e-10 of its minimum;
    a single candidate is the answer, and a row with several goes to all_pairs64.  Finite inputs."""
    s, t = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(tgt, dtype=np.float64).reshape(-1, 3)
    assert np.isfinite(s).all() and np.isfinite(t).all() and len(t) and max(np.abs(s).max(initial=0.0), np.abs(t).max()) < 100.0
    approx = (s * s).sum(axis=1)[:, None] + (t * t).sum(axis=1)[None, :] - 2.0 * (s @ t.T)
    idx = np.argmin(approx, axis=1)
    tied = np.nonzero((approx <= approx[np.arange(len(s)), idx][:, None] + 1e-10).sum(axis=1) > 1)[0]
    if len(tied):
        idx[tied] = nc.all_pairs64(s[tied], t)[1]
    return nc.true_d2(s, t, idx), idx


def _euler(x):
    (ca, cb, cg), (sa, sb, sg) = np.cos(x[:3]), np.sin(x[:3])
    R = np.array([[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa],
                  [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                  [-sb, cb * sa, cb * ca]])                                     # Rz(x2) Ry(x1) Rx(x0), multiplied out
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, x[3:6]
    return T


def icp_loop64(src, tgt, normals, max_dist, init=None, kind="point_to_plane", tukey_k=None, max_iteration=30,
               relative_fitness=1e-6, relative_rmse=1e-6):
    """Open3D's registration_icp in float64 numpy with exact float64 all-pairs correspondences, written out
    directly (nearest64 = nn_cases.all_pairs64's answer): J^T W J by a matrix product, Umeyama on the centred pairs.
    -> (T, fitness, inlier_rmse, iterations, [T after every evaluation])"""
    s, t = np.asarray(src, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)

    def evaluate(T):
        p = apply64(T, s)
        d2, idx = nearest64(p, t)
        inl = (idx >= 0) & (d2 <= max_dist * max_dist)
        fit = inl.sum() / len(s)
        rmse = math.sqrt(d2[inl].sum() / inl.sum()) if inl.any() else 0.0
        return p[inl], idx[inl], fit, rmse

    p, j, fit, rmse = evaluate(T)
    trace, its = [T.copy()], 0
    for _ in range(max_iteration):
        if len(p) == 0:
            break
        q = t[j]
        if kind == "point_to_plane":
            n = np.asarray(normals, dtype=np.float64)[j]
            r = ((p - q) * n).sum(axis=1)
            J = np.concatenate([np.cross(p, n), n], axis=1)
            w = np.ones(len(p))
            if tukey_k is not None:
                w = np.where(np.abs(r) <= tukey_k, (1.0 - (r / tukey_k) ** 2) ** 2, 0.0)
            A, b = J.T @ (J * w[:, None]), J.T @ (w * r)
            if np.linalg.matrix_rank(A) < 6:
                break
            U = _euler(np.linalg.solve(A, -b))
        else:
            pm, qm = p.mean(axis=0), q.mean(axis=0)
            Uu, _, Vt = np.linalg.svd((q - qm).T @ (p - pm) / len(p))
            S = np.diag([1.0, 1.0, np.sign(np.linalg.det(Uu) * np.linalg.det(Vt))])
            U = np.eye(4)
            U[:3, :3] = Uu @ S @ Vt
            U[:3, 3] = qm - U[:3, :3] @ pm
        T = U @ T
        its += 1
        prev = (fit, rmse)
        p, j, fit, rmse = evaluate(T)
        trace.append(T.copy())
        if abs(prev[0] - fit) < relative_fitness and abs(prev[1] - rmse) < relative_rmse:
            break
    return T, fit, rmse, its, trace


class Index64:
    """What ops.IcpWorkspace reads of an ops.NearestIndex, for a cloud on the host"""

    def __init__(self, tgt):
        self.tgt = np.asarray(tgt)
        self.bound_min, self.bound_max = tuple(self.tgt.min(axis=0).tolist()), tuple(self.tgt.max(axis=0).tolist())


class Workspace64:
    """Stands in for ops.IcpWorkspace on the CPU: the transform, the search and the sums in float64"""

    def __init__(self, src, index, normals=None):
        self.src, self.index, self.normals, self.n = np.asarray(src, dtype=np.float64), index, normals, len(src)
        self.origin = tuple(0.5 * (a + b) for a, b in zip(index.bound_min, index.bound_max))

    def step(self, T, max_dist, kind="point_to_plane", tukey_k=None):
        moved = apply64(np.asarray(T, dtype=np.float64), self.src)
        d2, idx = nearest64(moved, self.index.tgt)
        return sums64(moved, d2, idx, self.index.tgt, self.normals, max_dist, kind, tukey_k, self.origin)[0]


# --------------------------------------------------------------------------- fixtures
def _without_pairs_near(points, radius, rel=1e-5, keep=None):
    """Drops one point of every pair whose distance lies within ``rel`` (relative) of ``radius``, then keeps the first
    ``keep`` rows: the selection is a function of the seed alone."""
    p = np.asarray(points, dtype=np.float64)
    drop = np.zeros(len(p), dtype=bool)
    for a in range(0, len(p), 512):
        d = np.sqrt(((p[a:a + 512, None, :] - p[None, :, :]) ** 2).sum(axis=2))
        i, j = np.nonzero(np.abs(d - radius) <= 2.0 * rel * radius)
        drop[np.maximum(i + a, j)] = True
    return np.nonzero(~drop)[0][:keep]


@functools.lru_cache(maxsize=None)
def fixture():
    """-> dict: tgt (6000, 3) fp32 with face normals ``normals`` (fp32), src (5000, 3) fp32 an independent sampling of the
    same shape moved by the inverse of ``pose`` (3 deg / 5 cm), so that ICP from the identity should return ``pose``.
    No two targets lie within relative 1e-5 of NORMALS_RADIUS of each other."""
    rng = np.random.default_rng(4101)
    t, tn = shape_surface(rng, 6200)
    t = t.astype(F32)
    keep = _without_pairs_near(t, NORMALS_RADIUS, keep=6000)
    assert len(keep) == 6000
    t, tn = t[keep], tn[keep]
    s, _ = shape_surface(rng, 5000)
    P = pose(3.0, 0.05)
    out = dict(tgt=t, normals=tn.astype(F32), src=apply64(np.linalg.inv(P), s).astype(F32), pose=P)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def exact_fixture():
    """The source is 5 000 of the target's own rows moved by the inverse of ``pose``: at the optimum every residual is
    zero up to the fp32 rounding of the source rows."""
    f = fixture()
    rng = np.random.default_rng(4102)
    rows = rng.permutation(len(f["tgt"]))[:5000]
    src = apply64(np.linalg.inv(f["pose"]), f["tgt"][rows]).astype(F32)
    src.setflags(write=False)
    return dict(f, src=src, rows=rows)


@functools.lru_cache(maxsize=None)
def placed_pairs():
    """Pairs at exactly max_dist = 0.25 and one fp32 step to either side of it, far from each other: with the identity
    pose p' = src and d2 = 0.0625 exactly for the first pair.  -> (src (3, 3), tgt (3, 3), max_dist)"""
    tgt = np.array([[1.0, 1.0, 1.0], [11.0, 1.0, 1.0], [21.0, 1.0, 1.0]], dtype=F32)
    src = tgt.copy()
    src[0, 1] = F32(1.25)                                                        # exactly at 0.25
    src[1, 1] = np.nextafter(F32(1.25), F32(2.0))                                # one step beyond
    src[2, 1] = np.nextafter(F32(1.25), F32(0.0))                                # one step inside
    return src, tgt, 0.25


@functools.lru_cache(maxsize=None)
def loop64_pass(name, kind, which):
    """icp_loop64 on fixture() ('independent') or exact_fixture() ('exact'): the 'coarse' pass from the identity with the
    L2 loss at COARSE, or the 'fine' pass from its result with Tukey's loss at FINE; computed once"""
    f = fixture() if name == "independent" else exact_fixture()
    if which == "coarse":
        return icp_loop64(f["src"], f["tgt"], f["normals"], COARSE, None, kind, None, 30)
    return icp_loop64(f["src"], f["tgt"], f["normals"], FINE, loop64_pass(name, kind, "coarse")[0], kind, TUKEY_K, 30)


def loop64(name, kind):
    return loop64_pass(name, kind, "fine")


@functools.lru_cache(maxsize=None)
def normals_reference():
    """normals64 of the fixture's targets among themselves at NORMALS_RADIUS, computed once"""
    f = fixture()
    return normals64(f["tgt"], f["tgt"], NORMALS_RADIUS)
