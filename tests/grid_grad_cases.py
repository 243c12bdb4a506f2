"""Inputs on which the grid gradient has ONE right answer in fp32, and that answer in float64.  CPU only (numpy).

The grid gradient is the linear map  grad[l][c][v] = sum_i w_iv * dfeat[i][l C + c]  over the eight corners v of sample
i's cell.  With align_corners=False and zero padding (csrc/trilinear.hpp) the continuous index of a sample is
ix = ((xn + 1) size - 1) / 2.  Here every bound length is a power of two and every coordinate sits on the dyadic lattice
x = bmin + len j / 2**k, so xn + 1 = 2 j / 2**k, ix = j size / 2**k - 1/2, the fraction and both weights per axis are exact
in fp32 for ANY integer size, and so is every product wx wy wz d in every association when d = m 2**e with |m| <= 3.
If on top of that all terms of a vertex fit one 24-bit window -- (|prefill| + sum |term|) / (lowest set bit of any term or
of the prefill) <= 2**24 -- every partial sum in every order is representable: atomics, matrix-core accumulation, epochs
and slices must all give the float64 sum, bit for bit.  `budget_bits` measures that window and `assert_budget` refuses a
case that exceeds it: 24 is the significand width of fp32, not a measurement.

Measured maxima of log2(sum|term| / q) over all vertices and channels, and with the accumulate tests' prefill
0.25 randint(-4, 4) in, log2((|prefill| + sum|term|) / q); levels as (Z,Y,X):

    case  levels                               C  n      k  cluster   bits   prefilled
    A     16^3 32^3 64^3                       8  20000  6  yes       17.3   17.3
    B     16^3 32^3 64^3                       8  20000  8  no        17.4   22.1
    C     (12,20,33) (48,3,100)                4  20011  5  yes       19.1   19.2
    D     32^3 64^3 128^3                      8  70001  7  yes       16.7   16.7
    E     (20,10,20) (100,52,100) (72,33,120)  4  30011  5  yes       20.3   20.3
    F     16^3 32^3 64^3                       8  16384  6  yes       17.0   (16.2 with the fused tests' rows)
    G     (16,16,16) (12,20,144)               4  16384  6  yes       16.9   (16.1)
    P     (8,5,8) (80,50,80)                   4  8192   5  yes       21.4   (20.6)

E is for the per-axis binning (25,13,25) (tiles along x, y, z), which only the matrix-core pull serves: every level has at
least 2/3 as many vertices as tiles on every axis (plan_grad's mc_reaches) and at most 8 vertices per tile and axis;
(20,10,20) has fewer vertices than tiles on every axis, (100,52,100) is divided by all three tile counts, (72,33,120) by
none.  F, G and P feed the fused backward and training kernels (tests/test_grid_grad_exact.py).
"""
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

PINNED = 7      # rows at the end of every batch: four on corners / faces of the bound, NaN, +inf, 1e30


@dataclass
class LevelRef:
    G: np.ndarray      # (C,Z,Y,X) float64: the gradient
    S: np.ndarray      # (C,Z,Y,X) float64: sum of |term|
    M: np.ndarray      # (Z,Y,X) int64: contributions (in-range corners of non-zero weight)
    q: np.ndarray      # (C,Z,Y,X) float64: smallest lowest-set-bit over the non-zero terms, inf where there is none


@dataclass
class DyadicCase:
    levels: List[Tuple[int, int, int]]      # (Z,Y,X)
    C: int
    bound: List[List[float]]                # rows x, y, z: [min, max]
    x: np.ndarray                           # (n,3) float32
    dfeat: np.ndarray                       # (n, L C) float32
    j: np.ndarray                           # (n,3) int64 lattice indices (meaningless for the three non-finite rows)
    scale: np.ndarray                       # (n,) float64: 2**e_i, the regional scale of row i
    ref: List[LevelRef]

    @property
    def n(self):
        return self.x.shape[0]


def lowest_set_bit(a: np.ndarray) -> np.ndarray:
    """Value of the lowest set bit of every finite float64 in `a`; inf for zeros."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    m, e = np.frexp(a)                                   # a = m 2**e, m in [0.5, 1): m 2**53 is an integer
    mant = (m * 9007199254740992.0).astype(np.int64)
    low = (mant & -mant).astype(np.float64)
    out = np.ldexp(low, e - 53)
    return np.where(a == 0.0, np.inf, out)


def _axis(x64: np.ndarray, bmin: float, bmax: float, size: int):
    """trilinear.hpp axis_coord + axis_cell in float64: base corner, the two weights, the two in-range flags."""
    length = bmax - bmin
    xn = 2.0 * (x64 - bmin) / length - 1.0
    pos = ((xn + 1.0) * size - 1.0) * 0.5
    f = np.minimum(np.maximum(np.floor(pos), -2.0), size + 1.0)
    nan = np.isnan(pos)
    f = np.where(nan, -2.0, f)
    i0 = f.astype(np.int64)
    w0 = (f + 1.0) - pos
    w1 = pos - f
    in0 = (i0 >= 0) & (i0 < size) & ~nan
    in1 = (i0 + 1 >= 0) & (i0 + 1 < size) & ~nan
    return i0, (w0, w1), (in0, in1)


def reference(levels: Sequence[Tuple[int, int, int]], C: int, bound, x: np.ndarray, dfeat: np.ndarray,
              skip=None) -> List[LevelRef]:
    """The grid gradient of rows `dfeat` (n, L C) at points `x` (n,3), per level, as a float64 scatter over the eight
    corners; with the per-vertex statistics the exactness budget is judged by.  skip(level, i0, j0, k0, corner) -> bool
    mask of samples whose corner is left out: for mutation checks of the tests that use this reference, never set by them."""
    x64 = np.asarray(x, dtype=np.float64)
    d64 = np.asarray(dfeat, dtype=np.float64)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for l, (Z, Y, X) in enumerate(levels):
            i0, wx, inx = _axis(x64[:, 0], bound[0][0], bound[0][1], X)
            j0, wy, iny = _axis(x64[:, 1], bound[1][0], bound[1][1], Y)
            k0, wz, inz = _axis(x64[:, 2], bound[2][0], bound[2][1], Z)
            V = Z * Y * X
            G = np.zeros((C, V)); S = np.zeros((C, V)); M = np.zeros(V, dtype=np.int64)
            q = np.full((C, V), np.inf)
            d = d64[:, l * C:(l + 1) * C]
            for corner in range(8):
                dx, dy, dz = corner & 1, (corner >> 1) & 1, corner >> 2
                ok = inx[dx] & iny[dy] & inz[dz]
                if skip is not None:
                    ok = ok & ~skip(l, i0, j0, k0, corner)
                w = (wx[dx] * wy[dy]) * wz[dz]
                ok = ok & (w != 0.0)
                rows = np.nonzero(ok)[0]
                v = ((k0[rows] + dz) * Y + (j0[rows] + dy)) * X + (i0[rows] + dx)
                M += np.bincount(v, minlength=V)
                for c in range(C):
                    term = w[rows] * d[rows, c]
                    G[c] += np.bincount(v, weights=term, minlength=V)
                    S[c] += np.bincount(v, weights=np.abs(term), minlength=V)
                    np.minimum.at(q[c], v, lowest_set_bit(term))
            out.append(LevelRef(G.reshape(C, Z, Y, X), S.reshape(C, Z, Y, X), M.reshape(Z, Y, X), q.reshape(C, Z, Y, X)))
    return out


def budget_bits(ref: LevelRef, prefill: Optional[np.ndarray] = None) -> float:
    """max over the vertices that receive a non-zero term of log2((|prefill| + S) / q), q covering the prefill's lowest
    bit as well.  Vertices without a term hold the prefill (or zero) untouched: nothing is summed there."""
    live = np.isfinite(ref.q)
    if not live.any():
        return 0.0
    S, q = ref.S, ref.q
    if prefill is not None:
        p = np.asarray(prefill, dtype=np.float64).reshape(S.shape)
        S = S + np.abs(p)
        q = np.minimum(q, lowest_set_bit(p))
    return float(np.log2(S[live] / q[live]).max())


def assert_budget(refs: Sequence[LevelRef], prefills: Optional[Sequence[Optional[np.ndarray]]] = None) -> float:
    """Refuses inputs on which fp32 sums could depend on their order; returns the largest window in bits."""
    worst = 0.0
    for l, r in enumerate(refs):
        bits = budget_bits(r, None if prefills is None else prefills[l])
        assert bits <= 24.0, f"level {l}: terms of one vertex span {bits:.1f} bits: fp32 sums there depend on their order"
        worst = max(worst, bits)
    return worst


def lattice_points(bound, j: np.ndarray, k: int) -> np.ndarray:
    """x = bmin + len j / 2**k in fp32 (exact: every len is a power of two)."""
    b = np.asarray(bound, dtype=np.float64)
    length = b[:, 1] - b[:, 0]
    assert all(np.frexp(v)[0] == 0.5 for v in length), "bound lengths must be powers of two"
    x = (b[:, 0] + length * j.astype(np.float64) / float(2 ** k)).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), b[:, 0] + length * j / float(2 ** k))
    return x


def regional_scale(jx: np.ndarray, k: int) -> np.ndarray:
    """2**e, e = clamp(2 floor(8 j_x / K) - 8, -10, 8): a factor of four from region to region along x."""
    e = np.clip(2 * np.floor_divide(8 * jx, 2 ** k) - 8, -10, 8)
    return np.ldexp(1.0, e.astype(np.int64))


def dyadic_case(levels, C: int, bound, n: int, k: int, cluster: bool, seed: int) -> DyadicCase:
    rs = np.random.RandomState(seed)
    K = 2 ** k
    j = rs.randint(-K // 8, K + K // 8 + 1, size=(n, 3)).astype(np.int64)
    if cluster:
        j[: n // 4] = K // 2 + rs.randint(-K // 16, K // 16 + 1, size=(n // 4, 3))
    p = n - PINNED
    j[p + 0] = 0
    j[p + 1] = K
    j[p + 2] = K // 2
    j[p + 3] = (0, K, K // 2)
    x = lattice_points(bound, j, k)
    x[p + 4] = np.nan
    x[p + 5] = np.inf
    x[p + 6] = 1e30
    scale = regional_scale(j[:, 0], k)
    m = rs.randint(-3, 4, size=(n, C * len(levels)))
    m[p + 4:, 0] = 3                                     # the non-finite rows carry non-zero cotangents
    dfeat = (m * scale[:, None]).astype(np.float32)
    levels = [tuple(int(v) for v in lv) for lv in levels]
    case = DyadicCase(levels, C, [list(map(float, b)) for b in bound], x, dfeat, j, scale,
                      reference(levels, C, bound, x, dfeat))
    assert_budget(case.ref)
    return case


UNIT = [[-1.0, 1.0]] * 3
SPECS = {
    "A": dict(levels=[(16,) * 3, (32,) * 3, (64,) * 3], C=8, bound=UNIT, n=20000, k=6, cluster=True, seed=101),
    "B": dict(levels=[(16,) * 3, (32,) * 3, (64,) * 3], C=8, bound=UNIT, n=20000, k=8, cluster=False, seed=102),
    "C": dict(levels=[(12, 20, 33), (48, 3, 100)], C=4, bound=[[-2.0, 2.0], [0.0, 1.0], [-4.0, 4.0]], n=20011, k=5,
              cluster=True, seed=303),
    "D": dict(levels=[(32,) * 3, (64,) * 3, (128,) * 3], C=8, bound=UNIT, n=70001, k=7, cluster=True, seed=104),
    "E": dict(levels=[(20, 10, 20), (100, 52, 100), (72, 33, 120)], C=4, bound=[[-4.0, 4.0], [-1.0, 1.0], [-2.0, 2.0]],
              n=30011, k=5, cluster=True, seed=105),
    # A's grid with a power-of-two batch: d loss / d sdf of a mean loss, +-w_i / n, is then dyadic (the training kernels)
    "F": dict(levels=[(16,) * 3, (32,) * 3, (64,) * 3], C=8, bound=UNIT, n=16384, k=6, cluster=True, seed=106),
    # 144 vertices over 16 tiles are 9 a tile: beyond what the pull owns, so the fused kernels scatter that level themselves
    "G": dict(levels=[(16, 16, 16), (12, 20, 144)], C=4, bound=[[-4.0, 4.0], [0.0, 2.0], [-1.0, 1.0]], n=16384, k=6,
              cluster=True, seed=107),
    # a tile's samples reach <= 5 vertices per axis of the coarse level: the matrix-core push takes it under MISO_F_CROWDED;
    # up to 6 of the fine one, which stays with the pull
    "P": dict(levels=[(8, 5, 8), (80, 50, 80)], C=4, bound=[[-2.0, 2.0], [-1.0, 1.0], [-2.0, 2.0]], n=8192, k=5,
              cluster=True, seed=108),
}
TILES_E = (25, 13, 25)      # tiles along x, y, z
_CACHE = {}


def case(name: str) -> DyadicCase:
    """The named case, built once per process and shared: callers must not write into its arrays."""
    if name not in _CACHE:
        c = dyadic_case(**SPECS[name])
        for a in (c.x, c.dfeat, c.j, c.scale, *(t for r in c.ref for t in (r.G, r.S, r.M, r.q))):
            a.setflags(write=False)
        _CACHE[name] = c
    return _CACHE[name]


def prefill_pattern(shape, seed: int) -> np.ndarray:
    """0.25 randint(-4, 4): what the accumulate-mode tests put into the gradient buffers first."""
    return (0.25 * np.random.RandomState(seed).randint(-4, 5, size=shape)).astype(np.float32)
