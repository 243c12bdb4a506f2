"""References for the k-nearest-neighbour tests (tests/test_knn_host.py, tests/test_knn.py): the rule of csrc/knn.hip restated
in numpy fp32 (``knn32``), the true k nearest in float64 (``knn64``) and normals of a given neighbour set by
numpy.linalg.eigh (``knn_normals64``).  The clouds are those of nn_cases and icp_cases, plus the few sizes they lack.
Nothing here touches the library; every cloud is generated, none is stored."""
import functools

import numpy as np

import icp_cases as ic
import nn_cases as nc

F32 = np.float32
KS = (1, 2, 7, 30, 32)
K_NORMALS = 30


# --------------------------------------------------------------------------- references
def d2_32(src, tgt):
    """(N, M) fp32: ((ax - bx)^2 + (ay - by)^2) + (az - bz)^2, one rounding per operation (nn_cases.ring0_fp32's order);
    +inf where the result is not finite"""
    s, t = np.asarray(src, dtype=F32).reshape(-1, 3), np.asarray(tgt, dtype=F32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (s[:, None, :] - t[None, :, :]).astype(F32)
        d2 = ((d[..., 0] * d[..., 0]).astype(F32) + (d[..., 1] * d[..., 1]).astype(F32)).astype(F32)
        d2 = (d2 + (d[..., 2] * d[..., 2]).astype(F32)).astype(F32)
    return np.where(np.isfinite(d2), d2, F32(np.inf)).astype(F32)


def _k_smallest(d2, k):
    """the k smallest (value, column) pairs of every row, ascending; a stable sort: ties go to the lowest column.
    Slots whose value is +inf (or that do not exist) hold (+inf, -1)."""
    n, m = d2.shape
    D, I = np.full((n, k), np.inf, dtype=d2.dtype), np.full((n, k), -1, dtype=np.int64)
    if m:
        order = np.argsort(d2, axis=1, kind="stable")[:, :k]
        vals = np.take_along_axis(d2, order, axis=1)
        w = order.shape[1]
        D[:, :w] = vals
        I[:, :w] = np.where(np.isfinite(vals), order, -1)
    return D, I


def knn32(src, tgt, k, chunk=1024):
    """The rule of csrc/knn.hip in numpy fp32 -> (d2 (N, k) fp32, idx (N, k) int64)"""
    s = np.asarray(src, dtype=F32).reshape(-1, 3)
    out = [_k_smallest(d2_32(s[a:a + chunk], tgt), k) for a in range(0, len(s), chunk)]
    if not out:
        return np.zeros((0, k), dtype=F32), np.zeros((0, k), dtype=np.int64)
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def knn64(src, tgt, k, chunk=512):
    """The k smallest TRUE squared distances (float64 on the given fp32 values) and their indices, ties to the lowest
    index; rows with a non-finite coordinate match nothing -> (D (N, k) float64, idx (N, k))"""
    s, t = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(tgt, dtype=np.float64).reshape(-1, 3)
    out = []
    for a in range(0, len(s), chunk):
        with np.errstate(invalid="ignore", over="ignore"):
            d = s[a:a + chunk, None, :] - t[None, :, :]
            d2 = (d[..., 0] ** 2 + d[..., 1] ** 2) + d[..., 2] ** 2
        out.append(_k_smallest(np.where(np.isfinite(d2), d2, np.inf), k))
    if not out:
        return np.zeros((0, k)), np.zeros((0, k), dtype=np.int64)
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def true_d2(src, tgt, idx):
    """float64 squared distance of query i to each of idx[i, :] (inf where idx < 0)"""
    s, t = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(tgt, dtype=np.float64).reshape(-1, 3)
    idx = np.asarray(idx)
    out = np.full(idx.shape, np.inf)
    if idx.size and len(t):
        with np.errstate(invalid="ignore", over="ignore"):
            d = s[:, None, :] - t[np.maximum(idx, 0)]
            d2 = (d[..., 0] ** 2 + d[..., 1] ** 2) + d[..., 2] ** 2
        out = np.where(idx >= 0, d2, np.inf)
    return out


def knn_normals64(tgt, pts, idx):
    """For every row of pts the normal of the neighbour set idx[i] (rows of tgt; -1 = none): float64 covariance of
    d = t - q, numpy.linalg.eigh's eigenvector of the smallest eigenvalue, and the eigen-gap (l1 - l0) / l2.  Fewer than
    three neighbours: (0, 0, 1), gap 0.  -> (normals (N, 3), counts (N,), gaps (N,))"""
    t, q = np.asarray(tgt, dtype=np.float64).reshape(-1, 3), np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    idx = np.asarray(idx)
    normals, counts, gaps = np.tile([0.0, 0.0, 1.0], (len(q), 1)), (idx >= 0).sum(axis=1), np.zeros(len(q))
    for i in np.nonzero(counts >= 3)[0]:
        nb = t[idx[i][idx[i] >= 0]] - q[i]
        c = nb - nb.mean(axis=0)
        vals, vecs = np.linalg.eigh(c.T @ c / len(nb))
        normals[i] = vecs[:, 0]
        gaps[i] = (vals[1] - vals[0]) / vals[2] if vals[2] > 0 else 0.0
    return normals, counts, gaps


# --------------------------------------------------------------------------- clouds
def _cloud(m, n, seed):
    rng = np.random.default_rng(seed)
    return dict(tgt=rng.random((m, 3)), src=rng.random((n, 3)), cell=0.1, max_rings=4)


# the sizes nn_cases lacks: a full second block of queries, and target counts around k = 30
_EXTRA = {"n256": lambda: _cloud(1031, 256, 1556), "n0": lambda: _cloud(1031, 0, 1500),
          **{f"m{m}": (lambda m=m: _cloud(m, 70, 1600 + m)) for m in (0, 1, 2, 29, 30, 31)}}
N_NAMES = ("n0", "one_query", "n63", "n64", "n65", "n255", "n256", "n257")
M_NAMES = tuple(f"m{m}" for m in (0, 1, 2, 29, 30, 31))
NAMES = nc.NAMES + tuple(_EXTRA)


@functools.lru_cache(maxsize=None)
def case(name):
    """nn_cases.case, or one of the extra sizes: dict(tgt (M, 3) fp32, src (N, 3) fp32, cell, max_rings), read-only"""
    if name not in _EXTRA:
        return nc.case(name)
    c = _EXTRA[name]()
    for k in ("tgt", "src"):
        c[k] = np.ascontiguousarray(c[k], dtype=F32).reshape(-1, 3)
        c[k].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference32(name, k):
    c = case(name)
    D, I = knn32(c["src"], c["tgt"], k)
    D.setflags(write=False)
    I.setflags(write=False)
    return D, I


@functools.lru_cache(maxsize=None)
def reference64(name, k):
    c = case(name)
    D, I = knn64(c["src"], c["tgt"], k)
    D.setflags(write=False)
    I.setflags(write=False)
    return D, I


@functools.lru_cache(maxsize=None)
def fixture_neighbours():
    """icp_cases.fixture()'s targets among themselves at K_NORMALS: (knn64's D with one more column -- the (k+1)-th
    distance --, knn64's idx (6000, k), knn32's d2 and idx), computed once"""
    t = ic.fixture()["tgt"]
    D, I = knn64(t, t, K_NORMALS + 1)
    d32, i32 = knn32(t, t, K_NORMALS)
    for a in (D, I, d32, i32):
        a.setflags(write=False)
    return D, I[:, :K_NORMALS], d32, i32


@functools.lru_cache(maxsize=None)
def fixture_normals():
    """knn_normals64 of the fixture's targets on their float64 neighbour sets, computed once"""
    t = ic.fixture()["tgt"]
    return knn_normals64(t, t, fixture_neighbours()[1])
