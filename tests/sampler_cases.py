"""Inputs, oracle calls and bars of the first-order sampler tests: tests/test_sampler_first_order_host.py (CPU: the oracle
against fp64 ATen, the bars against fp32 restatements and planted faults) and tests/test_first_order_oracle.py (GPU:
every kernel form against the oracle).

Everything is evaluated at the kernel's own fp32 index coordinate (oracle.sample_index32), so a row planted on a cell
plane, a face or a clip limit is there for the kernel and for the oracle alike, and no finite row is left out.

Bars, per entry, u = 2^-24, each constant the number of roundings on the kernel's longest path to one term of the sum
the yardstick bounds (an fma only removes roundings), floor 1e-30:

  value, corner-weight form (encode_fwd_kernel, gather_level)      13 u sum_k |v_k| w_k
      3  the 1-D weights (f + 1) - ix and ix - f: exact by Sterbenz' lemma from cell 1 on, one rounding each in the
         cells next to index 0 (1 - ix for ix < 0.5, ix + 1 for ix in (-1, 0));  2  (wx wy) wz;  1  v w;
      7  the sum of eight
  value, lerp-tree form (lerp_tree's f)                             12 u sum_k |v_k|, in-range corners
      per axis: the edge difference, t's own rounding, t x difference, the sum = 4, every intermediate bounded by the
      sum of the |v_k| it is made of and carried to the result with a factor <= 1: 3 axes x 4.  The lerp value is NOT
      bounded by sum |v_k| w_k (a difference of two large corners times a small t), hence the other yardstick.
  grad_x, corner-weight form (encode_bwd_kernel)                    (8C + 8) u A_w
      A_w = sum_levels |gscale mult| sum_c |gF_c| sum_k |v_ck| x (the other two axes' weights)
      1  gF v;  3  the derivative weight (two 1-D weights, their product);  1  d dw;  8C  the sum over corners and
      channels;  2  gscale x mult and the product with it;  1  the sum over two levels.  (The float4 kernel sums
      4-channel dot products: 2C + 11, below it.)
  grad_x, lerp-tree form (encode_bwd_x_kernel)                      (2C + 12) u A_c
      A_c = sum_levels |gscale mult| sum_k sum_c |gF_c| |v_ck|
      2C  d_k = <gF, v_k> (C products, C sums);  9  lerp_tree's fx (two differences, t's rounding and t x difference
      and the sum, twice: y and z);  2 + 1  the scale and the level sum as above.
The fp32 `mult` itself is replayed by the oracle (oracle.mult32), so its roundings are on both sides."""
import functools
from typing import NamedTuple

import torch

from oracle import ref_torch as R

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
FLOOR = 1e-30

GRIDS = {"odd": ((5, 6, 7), (3, 4, 9)), "dyadic": ((4, 4, 4), (8, 8, 8))}      # (Z, Y, X) per level
BOUNDS = {"normalized": None,
          "metric": ((-1.0, 1.3), (-0.7, 0.9), (0.0, 2.1)),
          "dyadic": ((-1.0, 1.0), (-0.5, 1.5), (0.0, 4.0))}
MODES = [(pad, ac) for pad in ("zeros", "border") for ac in (False, True)]
KINDS = ("interior", "planes", "faces", "fade", "beyond", "clip", "nonfinite", "far")
K = {name: i for i, name in enumerate(KINDS)}


def value_bar_weight(o):
    return 13 * U * o.value_w + FLOOR


def value_bar_lerp(o):
    return 12 * U * o.value_c + FLOOR


def grad_bar_weight(o, C):
    return (8 * C + 8) * U * o.grad_w + FLOOR


def grad_bar_lerp(o, C):
    return (2 * C + 12) * U * o.grad_c + FLOOR


def xyz(level):
    z, y, x = level
    return (x, y, z)


def features(grid, C, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    return [torch.randn(1, C, *lv, generator=g) for lv in GRIDS[grid]]


# --------------------------------------------------------------------------- #
# Points
# --------------------------------------------------------------------------- #
def index_axis(x, a, size, bound, ac):
    """The kernel's fp32 index coordinate of coordinate x on axis a (before the border clip), as fp64."""
    xn = x
    if bound is not None:
        full = torch.zeros(x.shape[0], 3, dtype=F32)
        full[:, a] = x
        xn = R.norm32(full, bound)[:, a]
    return R.index32(xn, size, ac).double()


def _x_of_index(t, a, size, bound, ac):
    xn = t * 2 / (size - 1) - 1 if ac else (2 * t + 1) / size - 1
    if bound is None:
        return xn
    lo, hi = bound[a]
    return lo + (xn + 1) / 2 * (hi - lo)


def solve_axis(target, a, size, bound, ac, side, reach=64):
    """fp32 coordinates on axis a whose kernel index coordinate is exactly ``target`` (side 0), the nearest one below
    it (side -1) or above it (side +1): a search over the fp32 neighbours of the fp64 inverse (the index is monotone
    in the coordinate).  -> (x (M,) fp32, found (M,) bool)."""
    x0 = _x_of_index(target.double(), a, size, bound, ac)
    scale = 1.0 if bound is None else (bound[a][1] - bound[a][0]) / 2
    h = torch.clamp(x0.abs(), min=scale) * 2.0 ** -25
    k = torch.arange(-reach, reach + 1, dtype=F64)
    cand = (x0[:, None] + k[None, :] * h[:, None]).float()                      # (M, 2 reach + 1), non-decreasing
    ix = index_axis(cand.reshape(-1), a, size, bound, ac).view_as(cand)
    t = target.double()[:, None]
    rows = torch.arange(cand.shape[0])
    if side == 0:
        hit = ix == t
        found, j = hit.any(1), hit.float().argmax(1)
    elif side < 0:
        below = ix < t
        j = below.sum(1) - 1
        found = (j >= 0) & (j < cand.shape[1] - 1)
    else:
        j = (ix <= t).sum(1)
        found = (j > 0) & (j < cand.shape[1])
    return cand[rows, j.clamp(0, cand.shape[1] - 1)], found


class Points(NamedTuple):
    x: torch.Tensor            # (N,3) fp32, metres (normalised coordinates where the bound is None)
    kind: torch.Tensor         # (N,) index into KINDS
    level: torch.Tensor        # (N,) the level a planted row was planted for, -1 otherwise
    axes: torch.Tensor         # (N,3) bool: the axes a planted row was planted on
    target: torch.Tensor       # (N,3) fp64: the index coordinate planted there (NaN elsewhere)
    side: torch.Tensor         # (N,) -1 / 0 / +1: below, exactly at, above the target


@functools.lru_cache(maxsize=None)
def points(grid, bname, ac, n_interior=900):
    """The concatenated point set of one grid, bound and align_corners (the padding changes what is expected of a row,
    not where it is), a few hundred rows of each of KINDS: interior -- uniform in 1.15 x the bound; planes -- an exact
    integer index coordinate on one, two and three axes of each level; faces -- xn = -1 / +1 exactly and the fp32
    neighbour either side; fade -- ix in [-1, 0) and (size - 1, size], where zero padding loses corners; beyond -- ix =
    -1 and size exactly and the nearest index beyond each; clip -- ix = 0 and size - 1 and the nearest index either side
    (border padding sets mult = 0 there); nonfinite -- NaN, +inf, -inf on one axis each; far -- 1e9, 3e9, -1e9."""
    bound = BOUNDS[bname]
    levels = [xyz(lv) for lv in GRIDS[grid]]
    g = torch.Generator().manual_seed(7 + 13 * len(grid) + 3 * len(bname) + int(ac))
    lo = torch.tensor([-1.0] * 3 if bound is None else [b[0] for b in bound], dtype=F64)
    hi = torch.tensor([1.0] * 3 if bound is None else [b[1] for b in bound], dtype=F64)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    xs, kinds, lvls, axs, tgts, sides = [], [], [], [], [], []

    def inner(n, s=0.8):
        return (mid + half * s * (torch.rand(n, 3, generator=g, dtype=F64) * 2 - 1)).float()

    def add(x, kind, level=-1, axes=None, target=None, side=0, keep=None):
        n = x.shape[0]
        axes = torch.zeros(n, 3, dtype=torch.bool) if axes is None else axes
        target = torch.full((n, 3), float("nan"), dtype=F64) if target is None else target
        side = torch.full((n,), side, dtype=torch.long)
        keep = torch.ones(n, dtype=torch.bool) if keep is None else keep
        xs.append(x[keep]), kinds.append(torch.full((int(keep.sum()),), K[kind])), axs.append(axes[keep])
        lvls.append(torch.full((int(keep.sum()),), level)), tgts.append(target[keep]), sides.append(side[keep])

    def plant(kind, level, a, target, side, rows):
        """rows inner points with axis a moved to the coordinate that solve_axis finds for target"""
        t = torch.full((rows,), float(target), dtype=F64) if not torch.is_tensor(target) else target
        x = inner(t.shape[0])
        xa, found = solve_axis(t, a, levels[level][a], bound, ac, side)
        x[:, a] = xa
        axes = torch.zeros(t.shape[0], 3, dtype=torch.bool)
        axes[:, a] = True
        tg = torch.full((t.shape[0], 3), float("nan"), dtype=F64)
        tg[:, a] = t
        add(x, kind, level, axes, tg, side, found)

    add(inner(n_interior, 1.15), "interior")
    for l, sz in enumerate(levels):
        # planes: an exact integer index coordinate on one, two and three axes of this level
        for n_axes in (1, 2, 3):
            rows = 120
            x = inner(rows)
            axes = torch.zeros(rows, 3, dtype=torch.bool)
            order = torch.rand(rows, 3, generator=g).argsort(1)
            axes[torch.arange(rows)[:, None], order[:, :n_axes]] = True
            tg = torch.full((rows, 3), float("nan"), dtype=F64)
            keep = torch.ones(rows, dtype=torch.bool)
            for a in range(3):
                t = torch.randint(0, sz[a], (rows,), generator=g).double()
                xa, found = solve_axis(t, a, sz[a], bound, ac, 0)
                x[:, a] = torch.where(axes[:, a], xa, x[:, a])
                tg[:, a] = torch.where(axes[:, a], t, tg[:, a])
                keep &= found | ~axes[:, a]
            add(x, "planes", l, axes, tg, 0, keep)
        for a in range(3):
            # where zero padding loses corners: ix in [-1, 0) and (size - 1, size]
            r = torch.rand(24, generator=g, dtype=F64)
            for t in (r - 1, sz[a] - r):
                x = inner(24)
                x[:, a] = _x_of_index(t, a, sz[a], bound, ac).float()
                add(x, "fade")
            # ix = -1 and size exactly, and the nearest index beyond each: no corner in range on that axis
            for t, side in ((-1, 0), (-1, -1), (sz[a], 0), (sz[a], 1)):
                plant("beyond", l, a, t, side, 8)
            # both clip limits of border padding, exactly and the nearest index either side
            for t in (0, sz[a] - 1):
                for side in (-1, 0, 1):
                    plant("clip", l, a, t, side, 8)
    one = torch.tensor(1.0, dtype=F32)
    for a in range(3):
        # the faces of the bound, xn = -1 and +1 exactly, and the neighbouring fp32 coordinate either side
        for face in (lo[a].float(), hi[a].float()):
            for x_a in (face, torch.nextafter(face, face - one), torch.nextafter(face, face + one)):
                x = inner(8)
                x[:, a] = x_a
                add(x, "faces")
        x = inner(3)
        x[:, a] = torch.tensor([float("nan"), float("inf"), float("-inf")])
        add(x, "nonfinite")
        x = inner(3)
        x[:, a] = torch.tensor([1e9, 3e9, -1e9])
        add(x, "far")
    return Points(torch.cat(xs), torch.cat(kinds), torch.cat(lvls), torch.cat(axs), torch.cat(tgts), torch.cat(sides))


def gout_rows(n, F, seed=0, one_hot_C=None):
    """Random cotangent rows over all F channels; one_hot_C: a single non-zero channel per level of C channels (a wrong
    feature offset then reads zeros)."""
    g = torch.Generator().manual_seed(2000 + seed)
    go = torch.randn(n, F, generator=g)
    if one_hot_C is not None:
        keep = torch.zeros(F, dtype=torch.bool)
        for l in range(F // one_hot_C):
            keep[l * one_hot_C + (l + 1) % one_hot_C] = True
        go = go * keep
    return go


# --------------------------------------------------------------------------- #
# Oracle
# --------------------------------------------------------------------------- #
def coords(feats, bound, x32, pad, ac, ignore=None):
    """per level (ix, mult) at the kernel's coordinate, None for an ignored level"""
    out = []
    for l, f in enumerate(feats):
        if ignore is not None and ignore[l]:
            out.append((None, None))
        else:
            out.append(R.sample_index32(x32, bound, (f.shape[4], f.shape[3], f.shape[2]), ac, pad))
    return out


def oracle(feats, bound, x32, gout, pad, ac, ignore=None):
    cs = coords(feats, bound, x32, pad, ac, ignore)
    return R.trilinear_first64(feats, [c[0] for c in cs], gout.double(), [c[1] for c in cs])


@functools.lru_cache(maxsize=None)
def case(grid, bname, C, pad, ac, one_hot=False):
    """(features, points, gout, oracle) of one configuration, computed once per process and left unchanged."""
    feats = features(grid, C)
    pts = points(grid, bname, ac)
    go = gout_rows(pts.x.shape[0], C * len(feats), seed=C, one_hot_C=C if one_hot else None)
    return feats, pts, go, oracle(feats, BOUNDS[bname], pts.x, go, pad, ac)


def plant_vertex(feats, where, value, level=1):
    """A copy of the levels with ``value`` in one vertex: "first" -- flat vertex 0 of level 0, every channel (the address
    an out-of-range corner loads); "face" -- a vertex on the x = 0 face of ``level``; "interior" -- one inside it;
    channel 0 only for the last two."""
    out = [f.clone() for f in feats]
    if where == "first":
        out[0][0, :, 0, 0, 0] = value
    else:
        _, _, d, h, w = out[level].shape
        z, y, x = (d // 2, h // 2, 0) if where == "face" else (d // 2, h // 2, w // 2)
        out[level][0, 0, z, y, x] = value
    return out


# --------------------------------------------------------------------------- #
# Comparison
# --------------------------------------------------------------------------- #
WORST = {}     # form -> worst |got - fp64| / bar seen in this process


def excess(got, ref, bar):
    """|got - ref| / bar on the entries where the oracle is finite (NaN where it is not), and whether the two non-finite
    sets are equal entry for entry."""
    got = got.detach().double().cpu()
    fin = torch.isfinite(ref)
    same_set = torch.equal(torch.isfinite(got), fin)
    r = torch.where(fin, (got - ref).abs() / torch.where(fin, bar, torch.ones_like(bar)), torch.full_like(ref, float("nan")))
    return r, same_set


def check(form, what, got, ref, bar):
    """Every finite entry within its bar, every non-finite entry of the oracle non-finite in ``got`` and no other."""
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} for {tuple(ref.shape)}"
    if ref.numel() == 0:
        return
    r, same_set = excess(got, ref, bar)
    fin = torch.isfinite(ref)
    if not same_set:
        g = torch.isfinite(got.detach().cpu())
        raise AssertionError(f"{what}: non-finite entries differ from the oracle's: {int((~g & fin).sum())} where the oracle "
                             f"is finite, {int((g & ~fin).sum())} finite where it is not (rows "
                             f"{torch.nonzero((g != fin).reshape(g.shape[0], -1).any(1)).flatten()[:8].tolist()})")
    worst = r[fin].max().item() if fin.any() else 0.0
    WORST[form] = max(WORST.get(form, 0.0), worst)
    if worst > 1.0:
        i = torch.nonzero(torch.nan_to_num(r) == worst)[0].tolist()
        raise AssertionError(f"{what}: |got - fp64| = {worst:.3f} x the bar at entry {i} "
                             f"({int((torch.nan_to_num(r) > 1).sum())} entries beyond it)")
