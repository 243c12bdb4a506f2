"""Hash-indexed levels (include/miso_hash.h): a numpy restatement of the row index, the dense grid a table stands for,
and the fp32 terms of the table gradient -- shared by tests/test_hash_host.py (CPU) and tests/test_hash_encode.py (GPU).

The table-gradient reference.  The kernel adds, per in-range corner k of point p and channel c, the ONE fp32 number
t = fl(gF[p, c] * w_k) with w_k = fl(fl(wx wy) wz) from the fp32 1-D weights of trilinear.hpp's axis_cell (no sum is
involved in forming t, so nothing can be contracted into an fma), in whatever order the atomics arrive.  corner_terms32
restates w_k step by step in fp32 at the kernel's own index coordinate (oracle.sample_index32); the reference gradient
of a row is the float64 sum of its t's, and an fp32 sum of m such numbers in any order is within m 2^-24 sum |t| of
it (one rounding per addition, each on a partial sum bounded by sum |t|) -- and equal to it for m = 1.
test_hash_host.py ties corner_terms32 to the oracle: its cells, in-range flags and weights reproduce
oracle.trilinear_first64's value on the dense grid within the value bar."""
import functools

import numpy as np
import torch

import sampler_cases as sc
from oracle import ref_torch as R

PRIME_Y, PRIME_Z = 2654435761, 805459861
U = 2.0 ** -24

# ((i, j, k), log2, row) -- Instant-NGP's spatial hash
KNOWN = (((1, 0, 0), 19, 1), ((0, 1, 0), 19, 489905), ((0, 0, 1), 19, 153493), ((1, 1, 1), 19, 339493),
         ((2047, 2047, 2047), 19, 285147), ((3, 2, 5), 10, 648), ((17, 23, 9), 6, 11))

# the equivalence tests: two levels (X, Y, Z) over sampler_cases' metric bound; at log2 6 every row of both collides,
# at log2 8 the first is dense-indexed (105 vertices) and the second puts up to 17 vertices on a row
DIMS = ((5, 7, 3), (23, 17, 9))
GRID, BOUND = "hash", "metric"
LOG2S = (6, 8)
CHANNELS = (1, 2, 4, 8)
SIZES = (0, 1, 63, 64, 65, 257)


def level_rows(dims, log2):
    """(rows, dense-indexed?) -- Python integers, so 2048^3 cannot overflow"""
    X, Y, Z = (int(v) for v in dims)
    dense = X * Y * Z <= 1 << log2
    return (X * Y * Z if dense else 1 << log2), dense


def row_index(i, j, k, dims, log2):
    """rows of vertices (i, j, k) (integer arrays) as int64"""
    X, Y, Z = (int(v) for v in dims)
    i, j, k = (np.asarray(v, dtype=np.int64) for v in (i, j, k))
    rows, dense = level_rows(dims, log2)
    if dense:
        return (k * Y + j) * X + i
    u = lambda v: v.astype(np.uint32)      # noqa: E731  (products wrap in uint32)
    with np.errstate(over="ignore"):
        h = (u(i) * np.uint32(1)) ^ (u(j) * np.uint32(PRIME_Y)) ^ (u(k) * np.uint32(PRIME_Z))
    return (h & np.uint32(rows - 1)).astype(np.int64)


def dense_from_table(table, dims, log2):
    """The dense (1, C, Z, Y, X) grid D[k, j, i, :] = T[row(i, j, k)] a table stands for."""
    X, Y, Z = dims
    k, j, i = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    rows = torch.from_numpy(row_index(i, j, k, dims, log2))
    return table[rows].permute(3, 0, 1, 2).unsqueeze(0).contiguous()


def tables(log2, C, seed=0, dims=DIMS):
    g = torch.Generator().manual_seed(4000 + 10 * log2 + C + seed)
    return [torch.randn(level_rows(d, log2)[0], C, generator=g) for d in dims]


def corner_terms32(ix, dims, log2):
    """trilinear.hpp's axis_cell / corner_in / corner_weight<0> in fp32 at index coordinates ix (N,3) (fp32 values, any
    float dtype): -> (rows (N,8) int64 -- 0 where out of range, in-range (N,8) bool, w (N,8) float32)."""
    pos = np.asarray(ix, dtype=np.float64).astype(np.float32)
    n = pos.shape[0]
    i0, w, inr = [], [], []
    for a, size in enumerate(dims):
        p = pos[:, a]
        with np.errstate(invalid="ignore"):
            f = np.floor(p)
            f = np.where(np.isnan(f), np.float32(-2.0), np.minimum(np.maximum(f, np.float32(-2.0)), np.float32(size + 1)))
            f = f.astype(np.float32)
            base = np.where(np.isnan(p), -2, f.astype(np.int64))
            w.append(((f + np.float32(1.0)) - p, p - f))                     # one fp32 rounding each
        i0.append(base)
        inr.append(((base >= 0) & (base < size), (base + 1 >= 0) & (base + 1 < size)))
    rows = np.zeros((n, 8), dtype=np.int64)
    inb = np.zeros((n, 8), dtype=bool)
    wk = np.zeros((n, 8), dtype=np.float32)
    for k in range(8):
        o = (k & 1, (k >> 1) & 1, k >> 2)
        inb[:, k] = inr[0][o[0]] & inr[1][o[1]] & inr[2][o[2]]
        with np.errstate(invalid="ignore"):
            wk[:, k] = np.where(inb[:, k], (w[0][o[0]] * w[1][o[1]]) * w[2][o[2]], np.float32(0.0))
        c = [np.where(inb[:, k], i0[a] + o[a], 0) for a in range(3)]
        rows[:, k] = np.where(inb[:, k], row_index(c[0], c[1], c[2], dims, log2), 0)
    return rows, inb, wk


def table_gradient64(ix, dims, log2, gout, C, n_rows):
    """-> (float64 sum of the kernel's fp32 terms per table entry (rows, C), sum of their magnitudes, contributions m per
    row (rows,)); gout (N, C) float32: this level's columns of the cotangent."""
    rows, inb, wk = corner_terms32(ix, dims, log2)
    go = np.asarray(gout, dtype=np.float32)
    terms = (go[:, None, :] * wk[:, :, None]).astype(np.float32)           # (N,8,C): fl(gF w), one rounding
    ref, mag = np.zeros((n_rows, C)), np.zeros((n_rows, C))
    m = np.zeros(n_rows, dtype=np.int64)
    sel = inb.reshape(-1)
    r = rows.reshape(-1)[sel]
    np.add.at(ref, r, terms.reshape(-1, C).astype(np.float64)[sel])
    np.add.at(mag, r, np.abs(terms.reshape(-1, C).astype(np.float64))[sel])
    np.add.at(m, r, 1)
    return ref, mag, m


@functools.lru_cache(maxsize=None)
def points(ac=False):
    """sampler_cases.points planted for DIMS: interior, planes, faces, fade, beyond, clip, non-finite, far."""
    sc.GRIDS.setdefault(GRID, tuple((z, y, x) for x, y, z in DIMS))
    return sc.points(GRID, BOUND, ac, n_interior=300)


@functools.lru_cache(maxsize=None)
def subset(n):
    """n rows of points(), every kind among them: a fixed shuffle, None = all"""
    total = points().x.shape[0]
    if n is None:
        return torch.arange(total)
    return torch.randperm(total, generator=torch.Generator().manual_seed(31))[:n]


@functools.lru_cache(maxsize=None)
def case(log2, C, ignore=(False, False), pad="zeros", ac=False):
    """(tables, dense grids, points, cotangent, oracle on the dense grids) over all of points(ac): computed once per
    process and left unchanged; a test on a subset of the rows indexes the oracle's rows (they are per point)."""
    ts = tables(log2, C)
    ds = [dense_from_table(t, d, log2) for t, d in zip(ts, DIMS)]
    pts = points(ac)
    go = sc.gout_rows(pts.x.shape[0], C * len(ts), seed=C)
    return ts, ds, pts, go, sc.oracle(ds, sc.BOUNDS[BOUND], pts.x, go, pad, ac, ignore=list(ignore))


def index_coords(x32, dims, pad="zeros", ac=False):
    """the kernel's fp32 index coordinate of points x32 in a level of dims, as float64 (oracle.sample_index32)"""
    return R.sample_index32(x32, sc.BOUNDS[BOUND], dims, ac, pad)[0]
