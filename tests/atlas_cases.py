"""Atlases, points, oracle calls and bars of the fused atlas query tests: tests/test_atlas_host.py (CPU: the oracle against
fp64 autograd of the reference formula, the bars against an fp32 restatement and ten planted faults) and
tests/test_atlas_oracle.py (GPU: atlas_sdf_kernel and atlas_sdf_bwd_kernel against the oracle).

Membership and local coordinates are the kernels' own fp32 ones (oracle.atlas_to_submap32), so a row planted on a face of
a submap is on the same side for the kernel and for the oracle, and no finite row is left out.

Row order of every point set (it decides which wavefront a row lands in; every run below starts on a multiple of 64):
  [0, 64)      empty     wholly outside every submap
  [64, 128)    lonely    lane 0 at the centre of submap 0, the other 63 lanes far away
  [128, 192)   lonely    lane 63 at the centre of the last submap, the others far away
  [192, 256)   alone     NaN, +inf, -inf, 1e30 on one axis each (12 patterns, cycled): a run of non-finite rows only
  [256, 320)   mixed     interior rows with the 12 non-finite patterns on lanes 0, 5, 10, ... 55
  [320, 320+n) interior  uniform in the global bound plus a margin of 0.3
  then         faces     per submap its 8 corners, 12 edge midpoints and 6 face centres in the submap frame mapped to
                         world, each followed by its fp32 neighbour either side on every axis (7 rows per point)

Bars, per entry, u = 2^-24, floor 1e-30, bar = k u yardstick + floor (yardsticks: oracle.Atlas64).
  features   derived: every inside submap's value carries the 13 roundings of sampler_cases.value_bar_weight, the sum over
             the submaps count - 1 more, the division one: (13 + count) u sum_s value_w_s / count.
  sdf, gx, gposes, grid gradients, correction gradients   measured: k = 2 x (exact fp32 chains) or 4 x (bf16x3 split
             products) the worst |err| / (u yardstick) of loop32 below over all cases -- the package's per-submap loop
             under fp32 autograd on the CPU, fed the kernel's local coordinates -- the margins of
             test_split_precision.py and test_sphere_trace.py.  RESTATEMENT holds the measured ratios;
             test_atlas_host.py asserts that they still are what K was taken from.
  gposes     the kernel's addition depth exceeds the CPU sum's where few rows are inside a submap: per entry one product,
             6 shuffle steps over the wavefront, one LDS add per chunk the block works through (8 wavefronts a block at
             most, ceil(chunks / 2048) trips of the persistent loop: 256 blocks x 8 or 512 x 4), one rounding of the
             fp64 sum of the slots: 8 + 8 trips on top of the roundings of dxl itself, which gx (k_gx) bounds.
             k = max(measured, k_gx + 8 + 8 trips).
  corrections  the gradients of GridAtlas's rotation and translation corrections are the pose-table gradient pulled back
             through the table's construction: its bar pulled back the same way (k of gposes on the yardsticks |J|^T y)
             plus the measured k of the fp32 chain R0 Exp(dr), t0 + dt, [R^T, -R^T t] itself.
  grids      the scatter adds one term per row and corner with fp32 atomics, in any order: the same depth as the CPU's
             index_add in row order, so the measured k stands."""
import functools
import math
from typing import NamedTuple

import torch

from oracle import ref_torch as R
from sampler_cases import FLOOR, U, WORST, check  # noqa: F401  (one comparison and one table of worst ratios)

F32, F64 = torch.float32, torch.float64
TIE = 1e-6
BOUND = [[-1.0, 1.0], [-0.5, 0.75], [-1.0, 1.0]]
KINDS = ("empty", "lonely", "alone", "mixed", "interior", "faces")
K = {name: i for i, name in enumerate(KINDS)}
SIZES = (1, 63, 64, 65, 257, 513, 1025)
LATTICES = ((1, 1, 1), (2, 1, 33), (1, 65, 1))
# The persistent loops take a second trip beyond blocks x wavefronts x 64 points: atlas_sdf_kernel caps its grid at 2048
# blocks of 4 wavefronts (FwdLaunch, cap 2048: 2048 x 4 x 64 = 524288), atlas_sdf_bwd_kernel at 256 blocks of 8 wavefronts or 512
# of 4 (launch_atlas_bwd_t: 131072 either way).  + 65: one full chunk and a one-row chunk on the second trip.
N_STRIDE_FWD = 2048 * 4 * 64 + 65
N_STRIDE_BWD = 256 * 8 * 64 + 65
assert N_STRIDE_FWD == 524288 + 65 and N_STRIDE_BWD == 512 * 4 * 64 + 65 == 131072 + 65

# worst |loop32 - fp64| / (u yardstick) over all cases, per output (test_atlas_host.py measures them again).  The figures
# follow the CPU's math library; on two machines: sdf 0.151 / 0.160, gx 0.751 / 0.751, gposes 0.172 / 0.196, grids
# 1.727 / 1.727, and the corrections' fp32 chain, which holds an exponential map, 0.0046 / 0.0101.  The larger, rounded up.
RESTATEMENT = {"sdf": 0.16, "gx": 0.76, "gposes": 0.2, "grids": 1.75, "corrections": 0.011}
KBAR = {"exact_fp32": {k: 2 * v for k, v in RESTATEMENT.items()}, "split": {k: 4 * v for k, v in RESTATEMENT.items()}}


class Atlas(NamedTuple):
    name: str
    C: int
    L: int
    H: int
    feats: list          # per submap the levels (1,C,Z,Y,X) fp32
    bounds: list         # per submap (3,2)
    world: list          # per submap (R_world_submap (3,3), t_world_submap (3,)) fp64
    poses: torch.Tensor  # (S,12) fp32: R_submap_world row-major, t_submap_world
    ws: list
    bs: list
    ignore: object       # None, or per submap None / one bool per level
    locked: tuple        # submaps whose features take no gradient


def level_sizes(L, cells=None):
    """(Z, Y, X) per level, no axis longer than 32; cells: that many cells per axis on one level"""
    if cells is not None:
        return [(cells + 1,) * 3]
    return [(4 << l, (3 << l) + 1, (4 << l) - 1) for l in range(L)]


def rotation(rotvec):
    w = torch.tensor(rotvec, dtype=F64)
    th = w.norm().item()
    if th == 0:
        return torch.eye(3, dtype=F64)
    k = R.hat((w / th)[None])[0]
    return torch.eye(3, dtype=F64) + math.sin(th) * k + (1 - math.cos(th)) * (k @ k)


def build(name, C, L, H, world, bound=BOUND, cells=None, ignore=None, locked=(), seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    S, F_ = len(world), C * L
    feats = [[torch.randn(1, C, *lv, generator=g) for lv in level_sizes(L, cells)] for _ in range(S)]
    ws = [torch.randn(H, F_, generator=g) / math.sqrt(F_), torch.randn(H, H, generator=g) / math.sqrt(H),
          torch.randn(1, H, generator=g) / math.sqrt(H)]
    bs = [0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(1, generator=g)]
    # transfrom_points_from: x_local = R^T x_world - R^T t
    poses = torch.stack([torch.cat((Rw.t().reshape(-1), -(Rw.t() @ t))) for Rw, t in world]).to(F32)
    return Atlas(name, C, L, H, feats, [bound] * S, world, poses, ws, bs, ignore, tuple(locked))


def signed_permutation(perm, signs):
    m = torch.zeros(3, 3, dtype=F64)
    for r, (c, s) in enumerate(zip(perm, signs)):
        m[r, c] = s
    return m


GENERIC_ROTVECS = ((0.3, -0.2, 0.5), (-0.4, 0.1, 0.2), (0.2, 0.6, -0.3), (2.6, -0.9, 0.4), (-0.1, -0.5, -0.45))
GENERIC_CENTRE = (8.0, -6.0, 5.0)
GENERIC_OFFSETS = ((0.0, 0.0, 0.0), (0.3, 0.1, -0.2), (-0.25, 0.2, 0.15), (0.1, -0.15, 0.25), (-0.15, -0.25, -0.2))


@functools.lru_cache(maxsize=None)
def atlas(name):
    t64 = lambda v: torch.tensor(v, dtype=F64)
    if name == "exact":
        world = [(signed_permutation((0, 1, 2), (1, 1, 1)), t64([0.0, 0.0, 0.0])),
                 (signed_permutation((1, 0, 2), (-1, 1, 1)), t64([0.5, 0.25, 0.0])),
                 (signed_permutation((2, 1, 0), (1, -1, -1)), t64([-0.25, 0.5, 0.5])),
                 (signed_permutation((0, 2, 1), (-1, -1, -1)), t64([0.75, -0.5, 0.25]))]
        return build(name, 8, 3, 64, world, seed=1)
    if name.startswith("generic") or name in ("ignored", "locked"):
        world = [(rotation(w), t64(GENERIC_CENTRE) + t64(o)) for w, o in zip(GENERIC_ROTVECS, GENERIC_OFFSETS)]
        if name == "generic84":
            return build(name, 8, 4, 64, world, seed=2)
        ignore = [None, [False, True], None, [True, False], None] if name == "ignored" else None
        return build(name, 4, 2, 32, world, seed=3, ignore=ignore, locked=(2,) if name == "locked" else ())
    if name == "single":
        return build(name, 4, 1, 32, [(rotation((0.2, 0.1, -0.3)), t64([1.0, -2.0, 0.5]))], seed=4)
    if name == "pair":
        return build(name, 4, 1, 32, [(rotation((0.0, 0.0, 0.4)), t64([0.0, 0.0, 0.0])),
                                      (rotation((0.3, -0.2, 0.1)), t64([0.9, 0.2, -0.1]))], seed=5)
    if name == "many":
        world = [(rotation((0.0, 0.0, 0.02 * s)), t64([0.75 * s, 0.05 * (s % 3), 0.0])) for s in range(48)]
        return build(name, 4, 1, 32, world, bound=[[-0.5, 0.5]] * 3, cells=4, seed=6)
    raise KeyError(name)


def to_world(a, s, xl64):
    Rw, t = a.world[s]
    return xl64 @ Rw.t() + t


def global_bound(a):
    pts = []
    for s, b in enumerate(a.bounds):
        c = torch.tensor([[b[0][i & 1], b[1][(i >> 1) & 1], b[2][i >> 2]] for i in range(8)], dtype=F64)
        pts.append(to_world(a, s, c))
    pts = torch.cat(pts)
    return pts.min(0).values, pts.max(0).values


NONFINITE = [(a, v) for a in range(3) for v in (float("nan"), float("inf"), float("-inf"), 1e30)]


@functools.lru_cache(maxsize=None)
def points(name, n_interior):
    return points_of(atlas(name), n_interior, len(name) + 31 * n_interior)


def points_of(a, n_interior, seed):
    """-> (x (N,3) fp32, kind (N,)) in the row order of the module docstring"""
    g = torch.Generator().manual_seed(seed)
    lo, hi = global_bound(a)
    S = len(a.feats)

    def interior(n):
        return (lo - 0.3 + (hi - lo + 0.6) * torch.rand(n, 3, generator=g, dtype=F64)).float()

    def far(n):
        return (hi + 100.0 + 10.0 * torch.rand(n, 3, generator=g, dtype=F64)).float()

    def centre(s):
        b = torch.tensor(a.bounds[s], dtype=F64)
        return to_world(a, s, b.mean(1)[None]).float()[0]

    def poisoned(x, rows):
        for r, (axis, v) in zip(rows, NONFINITE):
            x[r, axis] = v
        return x

    lonely0, lonely63 = far(64), far(64)
    lonely0[0], lonely63[63] = centre(0), centre(S - 1)
    alone = interior(64)
    for r in range(64):
        alone[r, NONFINITE[r % 12][0]] = NONFINITE[r % 12][1]
    xs = [far(64), lonely0, lonely63, alone, poisoned(interior(64), range(0, 60, 5)), interior(n_interior)]
    kinds = [K["empty"]] * 64 + [K["lonely"]] * 128 + [K["alone"]] * 64 + [K["mixed"]] * 64 + [K["interior"]] * n_interior
    one = torch.tensor(1.0, dtype=F32)
    for s in range(S):
        b = a.bounds[s]
        marks = [[b[ax][0], 0.5 * (b[ax][0] + b[ax][1]), b[ax][1]] for ax in range(3)]
        local = torch.tensor([[marks[0][i], marks[1][j], marks[2][k]] for i in range(3) for j in range(3) for k in range(3)
                              if (i, j, k) != (1, 1, 1)], dtype=F64)
        w = to_world(a, s, local).float()                                             # (26,3)
        rows = [w]
        for ax in range(3):
            for step in (-one, one):
                nb = w.clone()
                nb[:, ax] = torch.nextafter(w[:, ax], w[:, ax] + step)
                rows.append(nb)
        xs.append(torch.stack(rows, 1).reshape(-1, 3))                                # point, then its six neighbours
        kinds += [K["faces"]] * (26 * 7)
    return torch.cat(xs), torch.tensor(kinds)


class Case(NamedTuple):
    name: str
    atlas: Atlas
    x: torch.Tensor          # (N,3) fp32
    kind: torch.Tensor       # (N,) index into KINDS
    gsdf: torch.Tensor       # (N,) fp32 cotangent of the SDF, zero on the tie rows
    o: R.Atlas64


def oracle(a, x, gsdf, **kw):
    return R.atlas64(a.feats, a.bounds, a.poses, x, a.ws, a.bs, gsdf, ignore=a.ignore, locked=a.locked, tie=TIE, **kw)


CASE_ATLAS = {"exact": ("exact", 1024), "generic84": ("generic84", 4096), "generic42": ("generic42", 4096),
              "single": ("single", 512), "many": ("many", 1024), "ignored": ("ignored", 1024), "locked": ("locked", 1024)}
SMALL_CASES = tuple(CASE_ATLAS) + tuple(f"n{n}" for n in SIZES)
STRIDE_CASES = ("stride_bwd", "stride_fwd")


@functools.lru_cache(maxsize=None)
def case(name):
    """One case, computed once per process and left unchanged.  n<k>: the first k rows of a fixed shuffle of generic42's
    points; stride_*: uniform rows on the two-submap atlas, enough for a second trip of the persistent loop."""
    g = torch.Generator().manual_seed(7 + sum(map(ord, name)))
    if name in CASE_ATLAS:
        a = atlas(CASE_ATLAS[name][0])
        x, kind = points(*CASE_ATLAS[name])
    elif name.startswith("n"):
        a = atlas("generic42")
        x, kind = points("generic42", 4096)
        perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(11))[:int(name[1:])]
        x, kind = x[perm], kind[perm]
    else:
        a = atlas("pair")
        n = N_STRIDE_BWD if name == "stride_bwd" else N_STRIDE_FWD
        lo, hi = global_bound(a)
        x = (lo - 0.3 + (hi - lo + 0.6) * torch.rand(n, 3, generator=g, dtype=F64)).float()
        kind = torch.full((n,), K["interior"])
    return make_case(name, a, x, kind, g)


def make_case(name, a, x, kind, g):
    """random cotangents, zero on the tie rows, and the oracle's answer to them"""
    o = oracle(a, x, torch.randn(x.shape[0], generator=g), zero_ties=True)
    return Case(name, a, x, kind, o.gsdf.float(), o)


# --------------------------------------------------------------------------- #
# GridAtlas itself: the generic poses with non-zero corrections, and the pull-back of the table gradient to them
# --------------------------------------------------------------------------- #
def module_atlas(device):
    """GridAtlas of five (4,2,32) submaps at the generic poses, random features and decoder, every submap and pose
    correction unlocked and the corrections away from zero (the exponential map's derivative is not the identity's).
    Every value comes from one CPU generator, so the atlas is the same on every device."""
    from miso_amd.grid_opt.models.grid_atlas import GridAtlas
    cfg = {"name": "grid_net", "spatial_dim": 3,
           "decoder": {"type": "mlp", "hidden_dim": 32, "hidden_layers": 1, "out_dim": 1, "pos_invariant": True,
                       "fix": True, "pretrained_model": None},
           "grid": {"type": "regular", "feature_dim": 4, "init_stddev": 3e-2, "bound": BOUND, "base_cell_size": 0.25,
                    "per_level_scale": 2, "n_levels": 2},
           "pose": {"optimize": False, "num_poses": 1}}
    m = GridAtlas(cfg, device=device)
    for w, off in zip(GENERIC_ROTVECS, GENERIC_OFFSETS):
        t = torch.tensor(GENERIC_CENTRE, dtype=F64) + torch.tensor(off, dtype=F64)
        m.add_submap(torch.tensor(BOUND), rotation(w).float(), t.float()[:, None], num_poses=1)
        m.add_kf(torch.eye(3), torch.zeros(3, 1))
    m = m.to(device)
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():
        for sm in m.submaps:
            for grid in sm.features:
                grid.feature.copy_(torch.randn(grid.feature.shape, generator=g))
            for p in sm.decoder.parameters():
                p.copy_(torch.randn(p.shape, generator=g) / math.sqrt(p.shape[-1]) if p.ndim == 2 else
                        0.1 * torch.randn(p.shape, generator=g))
        for s in range(m.num_submaps):
            m.rotation_corrections[s].copy_(0.05 * torch.randn(1, 3, generator=g))
            m.translation_corrections[s].copy_(0.05 * torch.randn(3, 1, generator=g))
    for s in range(m.num_submaps):
        m.unlock_submap(s)
    m.unlock_submap_pose()
    return m


def as_atlas(m, table):
    """the atlas_cases.Atlas of a GridAtlas; table: the (S,12) pose table its kernels are handed (GridAtlas._pose_table)"""
    feats = [[grid.feature.detach().cpu().contiguous() for grid in sm.features] for sm in m.submaps]
    world = []
    with torch.no_grad():
        for s in range(m.num_submaps):
            Rw, t = m.updated_submap_pose(s)
            world.append((Rw.detach().cpu().double(), t.detach().cpu().double()[:, 0]))
    ws, bs = R.decoder_params({k: v.detach().cpu() for k, v in m.submaps[0].decoder.state_dict().items()})
    C, L, H = feats[0][0].shape[1], len(feats[0]), ws[0].shape[0]
    return Atlas("module", C, L, H, feats, [BOUND] * len(feats), world, table.detach().cpu().float(), ws, bs, None, ())


def corrections(m, gposes, gposes_y=None, dtype=F64):
    """The (S,12) pose-table gradient pulled back to the corrections through a copy of GridAtlas._pose_table in
    ``dtype``: R = R0 Exp(dr), t = t0 + dt (apply_pose_correction), row = [R^T, -R^T t].  -> per submap (d dr (1,3),
    d dt (3,1)), and with gposes_y the yardsticks |J|^T gposes_y."""
    out, ys = [], []
    for s in range(m.num_submaps):
        R0, t0 = (t.detach().cpu().to(dtype) for t in m.initial_submap_pose(s))
        dr = m.rotation_corrections[s].detach().cpu().to(dtype)
        dt = m.translation_corrections[s].detach().cpu().to(dtype)

        def row(dr, dt):
            Rw, t = R.apply_pose_correction(R0, t0, dr, dt)
            return torch.cat((Rw.t().reshape(-1), -(Rw.t() @ t).reshape(-1)))

        J = torch.autograd.functional.jacobian(row, (dr, dt))
        g = gposes[s].detach().cpu().to(dtype)
        out.append((torch.einsum("i,iab->ab", g, J[0]), torch.einsum("i,iab->ab", g, J[1])))
        if gposes_y is not None:
            ys.append((torch.einsum("i,iab->ab", gposes_y[s], J[0].abs().double()),
                       torch.einsum("i,iab->ab", gposes_y[s], J[1].abs().double())))
    return (out, ys) if gposes_y is not None else out


def module_case(m, table):
    a = as_atlas(m, table)
    x, kind = points_of(a, 1024, 1234)
    return make_case("module", a, x, kind, torch.Generator().manual_seed(4321))


# --------------------------------------------------------------------------- #
# The fp32 restatement: the package's per-submap loop under fp32 autograd, on the CPU
# --------------------------------------------------------------------------- #
class Outputs(NamedTuple):
    feat: torch.Tensor
    sdf: torch.Tensor
    gx: torch.Tensor
    gposes: torch.Tensor
    grids: list


def sample32(feature, ix):
    """the zero-padded trilinear sample in the corner-weight form, every operation in the dtype of ix (fp32), at the
    index coordinates ix (N,3): differentiable in ix and in the feature"""
    _, ch, d, h, w = feature.shape
    flat = feature.reshape(ch, d * h * w)
    away = ((ix < -2) | (ix > max(w, h, d) + 1)).any(1)      # no corner in range: keep 1e30 away out of the weights
    ix = torch.where(away[:, None], torch.full_like(ix, -4.0), ix)
    i0 = torch.floor(ix).detach().clamp(-2, max(w, h, d) + 1)
    out = 0
    for k in range(8):
        o = (k & 1, (k >> 1) & 1, k >> 2)
        wt = [(ix[:, a] - i0[:, a]) if o[a] else (i0[:, a] + 1 - ix[:, a]) for a in range(3)]
        xi, yi, zi = (i0[:, a].long() + o[a] for a in range(3))
        inb = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h) & (zi >= 0) & (zi < d)
        lin = (zi.clamp(0, d - 1) * h + yi.clamp(0, h - 1)) * w + xi.clamp(0, w - 1)
        out = out + torch.where(inb[:, None], flat[:, lin].t(), torch.zeros((), dtype=ix.dtype)) * ((wt[0] * wt[1]) * wt[2])[:, None]
    return out


def loop32(c):
    """GridAtlas.query_feature / forward (grid_atlas.py: frame change, coords_in_bound, the multi-level sample of every
    row, mask x feats summed, count clamped, decoder) in fp32 with autograd behind it, on the finite rows.  Coordinates
    carry the VALUES the kernel forms -- the local coordinate of oracle.atlas_to_submap32 and the index coordinate of
    oracle.sample_index32: a one-ulp difference of either moves the sample by more than every rounding after it, and a
    row next to a cell plane into another cell -- and the derivatives of the fp32 matrix product and of gscale x mult.
    Non-finite rows: zero feature row, the zero-row SDF, zero gx (the loop itself answers NaN there)."""
    a, o = c.atlas, c.o
    S = len(a.feats)
    fin = torch.isfinite(c.x).all(1)
    x = c.x[fin].clone().requires_grad_(True)
    poses = a.poses.clone().requires_grad_(True)
    feats = [[f.clone().requires_grad_(s not in a.locked) for f in fs] for s, fs in enumerate(a.feats)]
    total, count = 0, 0
    for s in range(S):
        moved = x @ poses[s, :9].view(3, 3).t() + poses[s, 9:]
        xl32 = o.xl[s][fin]
        inside = R.coords_in_bound(xl32, torch.tensor(a.bounds[s], dtype=F32))
        rows = []
        for l, f in enumerate(feats[s]):
            if a.ignore is not None and a.ignore[s] is not None and a.ignore[s][l]:
                rows.append(torch.zeros(x.shape[0], f.shape[1]))
                continue
            ix, mult = R.sample_index32(xl32, a.bounds[s], (f.shape[4], f.shape[3], f.shape[2]))
            rows.append(sample32(f, ix.float() + mult.float() * (moved - moved.detach())))
        total = total + inside * torch.cat(rows, 1)
        count = count + inside
    count = count.float()
    count[count == 0] = 1
    mean = total / count
    sdf = R.mlp_forward(mean, a.ws, a.bs)
    (c.gsdf[fin, None] * sdf).sum().backward()
    n, F_ = c.x.shape[0], a.C * a.L
    feat, full, gx = torch.zeros(n, F_), torch.empty(n), torch.zeros(n, 3)
    full[:] = R.mlp_forward(torch.zeros(1, F_), a.ws, a.bs)[0, 0]
    feat[fin], full[fin], gx[fin] = mean.detach(), sdf.detach()[:, 0], x.grad
    grids = [[None if s in a.locked else (torch.zeros_like(f) if f.grad is None else f.grad) for f in fs]
             for s, fs in enumerate(feats)]
    return Outputs(feat, full, gx, poses.grad, grids)


# --------------------------------------------------------------------------- #
# Bars
# --------------------------------------------------------------------------- #
def feat_bar(o):
    return (13 + o.count.clamp(min=1).double())[:, None] * U * o.feat_y + FLOOR


def pose_depth(n):
    """additions on the kernel's path to one pose-gradient entry beyond the roundings of dxl: docstring"""
    chunks = (n + 63) // 64
    return 8 + 8 * ((chunks + 2047) // 2048)


def kbar(form, what, n=0):
    k = KBAR[form][what]
    if what == "gposes":
        k = max(k, KBAR[form]["gx"] + pose_depth(n))
    return k


def corrections_bars(form, n, ys):
    """the pose-table bar pulled back through |J| (the yardsticks already are), plus the fp32 chain's own roundings"""
    k = kbar(form, "gposes", n) + kbar(form, "corrections")
    return [(k * U * ya + FLOOR, k * U * yb + FLOOR) for ya, yb in ys]


def bars(c, form):
    """bar per output of case c for the decoder form ("exact_fp32" / "split"), in the layout of Outputs"""
    o, n = c.o, c.x.shape[0]
    return Outputs(feat_bar(o), kbar(form, "sdf") * U * o.sdf_y + FLOOR, kbar(form, "gx") * U * o.gx_y + FLOOR,
                   kbar(form, "gposes", n) * U * o.gposes_y + FLOOR,
                   [[None if y is None else kbar(form, "grids") * U * y + FLOOR for y in ys] for ys in o.grids_y])


def wanted(o):
    """the oracle's answers in the layout of Outputs"""
    return Outputs(o.feat, o.sdf, o.gx, o.gposes, o.grids)


def ratios(got, c):
    """worst |got - fp64| / (u yardstick) per output over the finite entries of the oracle (what K is measured with)"""
    o = c.o
    r = lambda g, w, y: ((g.double() - w).abs() / (U * y + FLOOR)).max().item() if w.numel() else 0.0  # noqa: E731
    out = {"sdf": r(got.sdf, o.sdf, o.sdf_y), "gx": r(got.gx, o.gx, o.gx_y), "gposes": r(got.gposes, o.gposes, o.gposes_y)}
    out["grids"] = max([r(g, w, y) for gs, ws, ys in zip(got.grids, o.grids, o.grids_y) for g, w, y in zip(gs, ws, ys)
                        if w is not None] + [0.0])
    return out


def check_outputs(form, what, got, c, fields=("feat", "sdf", "gx", "gposes", "grids")):
    """every asked output of ``got`` (Outputs; None: not formed) within its bar of the oracle, non-finite sets equal"""
    want, bar = wanted(c.o), bars(c, form)
    for f in fields:
        g = getattr(got, f)
        if f != "grids":
            check(f"atlas {f} ({form})", f"{what}/{f}", g, getattr(want, f), getattr(bar, f))
            continue
        for s, (gs, ws, bs) in enumerate(zip(g, want.grids, bar.grids)):
            for l, (gl, wl, bl) in enumerate(zip(gs, ws, bs)):
                assert (gl is None) == (wl is None), f"{what}: level gradient {s}/{l} formed for a locked submap, or missing"
                if wl is not None:
                    check(f"atlas grids ({form})", f"{what}/grid {s}/{l}", gl, wl, bl)


# --------------------------------------------------------------------------- #
# Planted faults: what a kernel with the fault would return, in fp64 (only the outputs the fault changes)
# --------------------------------------------------------------------------- #
FAULTS = {1: ("an exclusive upper bound", "exact"),
          2: ("membership decided in float64", "exact"),
          3: ("the mean divided by S instead of the count", "generic42"),
          4: ("the count not clamped at zero", "generic42"),
          5: ("the backward's d-feat row not divided by the count", "generic42"),
          6: ("R for R^T in gx", "generic42"),
          7: ("x_local for x_world in the rotation block of gposes", "generic42"),
          8: ("pose rows >= 43 left at zero", "many"),
          9: ("an ignored level still feeding dxl", "ignored"),
          10: ("one count per wavefront: every lane of a run counts the submaps ANY of its lanes is inside", "generic42")}


def inside64(a, x):
    """the membership of the literal formula in float64: (N,S)"""
    x = x.double()
    cols = []
    for s in range(len(a.feats)):
        Rw, t = a.world[s]
        xl = R.transfrom_points_from(x, Rw, t[:, None])
        cols.append(R.coords_in_bound(xl, torch.tensor(a.bounds[s], dtype=F64))[:, 0])
    return torch.stack(cols, 1)


def fault(k, c):
    """-> (Outputs with None for what the fault leaves alone)"""
    a, o = c.atlas, c.o
    S = len(a.feats)
    den = o.count.clamp(min=1).double()[:, None]
    none = Outputs(None, None, None, None, None)
    if k == 1:
        hi = torch.tensor(a.bounds, dtype=F32)[:, :, 1]
        return wanted(oracle(a, c.x, c.gsdf, inside=o.inside & (o.xl < hi[:, None, :]).all(2).t()))
    if k == 2:
        return wanted(oracle(a, c.x, c.gsdf, inside=inside64(a, c.x)))
    if k == 3:
        return none._replace(feat=o.feat * den / S)
    if k == 4:
        return none._replace(feat=torch.where((o.count == 0)[:, None], torch.full_like(o.feat, float("nan")), o.feat))
    if k == 5:
        w = wanted(oracle(a, c.x, c.gsdf.double() * den[:, 0]))
        return none._replace(gx=w.gx, gposes=w.gposes, grids=w.grids)
    if k == 6:
        return none._replace(gx=torch.einsum("skj,snj->nk", a.poses[:, :9].double().view(S, 3, 3), o.dxl))
    if k == 7:
        xl = torch.nan_to_num(o.xl.double(), 0.0, 0.0, 0.0)
        gp = o.gposes.clone()
        gp[:, :9] = torch.einsum("snj,snk->sjk", o.dxl, xl).reshape(S, 9)
        return none._replace(gposes=gp)
    if k == 8:
        gp = o.gposes.clone()
        gp[43:] = 0
        return none._replace(gposes=gp)
    if k == 9:
        gx = o.gx.clone()
        for s in range(S):
            c0 = 0
            for l, f in enumerate(a.feats[s]):
                ch = f.shape[1]
                if a.ignore is not None and a.ignore[s] is not None and a.ignore[s][l]:
                    ix, mult = R.sample_index32(o.xl[s], a.bounds[s], (f.shape[4], f.shape[3], f.shape[2]))
                    ix = torch.where(o.inside[:, s, None], ix, torch.full_like(ix, float("nan")))
                    der = R._trilinear_jet_select(f, ix)[1]
                    extra = mult * (o.dfeat[:, c0:c0 + ch, None] * der).sum(1)
                    gx += extra @ a.poses[s, :9].double().view(3, 3)
                c0 += ch
        return none._replace(gx=gx)
    if k == 10:
        n = c.x.shape[0]
        pad = (-n) % 64
        ins = torch.cat((o.inside, torch.zeros(pad, S, dtype=torch.bool)))
        per_run = ins.view(-1, 64, S).any(1).sum(1).repeat_interleave(64)[:n]
        return none._replace(feat=o.feat * den / per_run.clamp(min=1).double()[:, None])
    raise KeyError(k)


def rejected(form, got, c):
    """does some bar of case c reject ``got`` (Outputs, None where the fault changes nothing)?"""
    fields = [f for f in Outputs._fields if getattr(got, f) is not None]
    seen = dict(WORST)
    try:
        check_outputs(form, "fault", got, c, fields)
    except AssertionError:
        return True
    finally:
        WORST.clear()
        WORST.update(seen)      # (a planted fault is not a measurement)
    return False
