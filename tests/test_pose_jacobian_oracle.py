"""The pose-Jacobian path of latent alignment (pair_latent.hip, align.hip, ops._PairLatent / _PairLatentMulti /
AlignPlan) against fp64 oracles evaluated at the kernel's own fp32 mapped coordinates (oracle.ref_torch:
src_to_dst32, pair_latent_sums64, align_epilogue64, align_epilogue_b64).  Because the oracle takes the same cells and
the same in-bound set as the kernel, what is left is rounding:

* in-bound counts: exactly the src_to_dst32 count;
* every other pair sum: |kernel - fp64| <= 1e-5 A + 1e-12, A the same sum built from per-vertex absolute bounds
  (pair_latent_sums64's docstring; tests/test_alignment_oracle.py checks on the CPU that this bar rejects a dropped
  vertex, a wrong level offset, a flipped gradient sign on 1 % of the vertices and a count off by one);
* epilogue A (`flat`): 1e-6 of the same pull-back in absolute values, fed the kernel's own sums; against the full
  fp64 oracle, the per-sum bounds are pushed through that absolute-value map;
* epilogue B: Adam in fp32 against fp64 from the kernel's `flat`.
"""
import math

import numpy as np
import pytest
import torch

import golden_cases as gc
from oracle import ref_torch as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
REL = 1e-5
FAMILIES = {"term": [0], "G": [2, 3, 4], "d(x)g": list(range(5, 14)), "(Rd g)(x)p": list(range(14, 23))}
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """print the worst |kernel - fp64| / A per sum family over the cases that ran (recorded in DESIGN.md section 2);
    the bar itself is _check_sums'"""
    yield
    if _WORST:
        print("\nworst |kernel - fp64| / A:", {k: f"{v:.2e}" for k, v in _WORST.items()})


def _record(got, sums, A):
    """keep the worst |kernel - fp64| / A per sum family (printed by the last test of the module)"""
    got = torch.as_tensor(got, dtype=F64).cpu().reshape(24)
    for fam, ix in FAMILIES.items():
        a = A[ix]
        ok = a > 0
        if ok.any():
            r = ((got[ix] - sums[ix]).abs()[ok] / a[ok]).max().item()
            _WORST[fam] = max(_WORST.get(fam, 0.0), r)


def _check_sums(what, got, sums, A):
    got = torch.as_tensor(got, dtype=F64).cpu().reshape(24)
    ex = R.pair_sums_excess(got, sums, A, REL)
    _record(got, sums, A)
    bad = torch.nonzero(ex > 0).flatten().tolist()
    assert not bad, (f"{what}: sums {bad} beyond the bar; count kernel {got[1].item()} oracle {sums[1].item()}; "
                     f"|d| {(got - sums).abs()[bad].tolist()} A {A[bad].tolist()}")


# --------------------------------------------------------------------------- #
# Inputs
# --------------------------------------------------------------------------- #
BOUND = [[-4.0, 4.0], [-2.0, 3.0], [-3.0, 3.5]]
LEVEL_XYZ = [(7, 5, 6), (13, 9, 1), (25, 17, 11)]        # odd, non-cubic, one size-1 axis


def _levels(layout, nlev, g, xyz=LEVEL_XYZ, const=None):
    """destination levels on the device: cl4 / cl8 channels-last (the float4 kernel), nc4 / nc3 / nc1 NCDHW (scalar)"""
    c = {"cl4": 4, "cl8": 8, "nc4": 4, "nc3": 3, "nc1": 1}[layout]
    out = []
    for X, Y, Z in xyz[:nlev]:
        f = torch.randn(1, c, Z, Y, X, generator=g) * 0.1 if const is None else torch.full((1, c, Z, Y, X), const)
        out.append(f)
    dev = [f.to(DEV).contiguous(memory_format=torch.channels_last_3d) if layout.startswith("cl") else f.to(DEV)
           for f in out]
    return out, dev


def _rot(rs, scale=0.5):
    return torch.tensor(gc.rodrigues(rs.uniform(-scale, scale, 3)), dtype=F32)


def _pose(Rs, ts, Rd, td):
    return torch.cat([torch.as_tensor(v, dtype=F32).reshape(-1) for v in (Rs, ts, Rd, td)])


def _src_of(q, pose):
    """source vertices (fp32) whose exact map is q (fp64): p = Rs^T (Rd q + td - ts)"""
    p64 = pose.double()
    Rs, ts, Rd, td = p64[:9].view(3, 3), p64[9:12], p64[12:21].view(3, 3), p64[21:24]
    return ((q @ Rd.T + td - ts) @ Rs).float()


def _geometry(kind, n, g, rs):
    """(p (n,3) fp32, pose (24,), bound) for one geometry"""
    b = torch.tensor(BOUND, dtype=F64)
    if kind == "perm":
        # signed permutations, dyadic translations, vertices on a 1/16 m lattice: exact arithmetic, so vertices sit ON the
        # faces of the bound and on interior cell planes (power-of-two level sizes, see _run_pair)
        Rs = torch.tensor([[0., -1, 0], [0, 0, 1], [-1, 0, 0]])
        Rd = torch.tensor([[0., 0, 1], [1, 0, 0], [0, 1, 0]])
        ts, td = torch.tensor([0.5, -1.25, 2.0]), torch.tensor([-0.75, 0.125, 1.5])
        pose = _pose(Rs, ts, Rd, td)
        bound = [[-4.0, 4.0], [-2.0, 2.0], [-1.0, 3.0]]
        q = (torch.randint(-80, 81, (n, 3), generator=g).double() / 16) * torch.tensor([1.0, 0.5, 0.5]) + \
            torch.tensor([0.0, 0.0, 1.0])
        return _src_of(q, pose), pose, bound
    if kind == "far_t":                                   # translations of ~1e3 m
        Rs, Rd = _rot(rs), _rot(rs)
        ts = torch.tensor(rs.uniform(-1000, 1000, 3), dtype=F32)
        td = ts + torch.tensor(rs.uniform(-1, 1, 3), dtype=F32)
        pose = _pose(Rs, ts, Rd, td)
    elif kind.startswith("far_p"):                        # the destination bound ~1e3 (1e4) m from the origin: |p| ~ |q|
        off = 10000.0 if kind.startswith("far_p4") else 1000.0
        Rs, Rd = _rot(rs, 0.05), _rot(rs, 0.05)
        ts = torch.tensor(rs.uniform(-1, 1, 3), dtype=F32)
        td = torch.tensor(rs.uniform(-1, 1, 3), dtype=F32)
        pose = _pose(Rs, ts, Rd, td)
        bound = [[off - 4.0, off + 4.0], [-2.0, 3.0], [off - 3.0, off + 3.5]]
        bb = torch.tensor(bound, dtype=F64)
        q = (torch.rand(n, 3, generator=g, dtype=F64) * 1.2 - 0.1) * (bb[:, 1] - bb[:, 0]) + bb[:, 0]
        if kind.endswith("_band"):
            # every vertex within 6e-3 m of a face (either side): at 1e4 m one fp32 ulp is 9.8e-4 m, so the rounding of
            # the pass-1 composed map and of the exact map is a good part of the band
            ax = torch.randint(0, 3, (n,), generator=g)
            side = torch.randint(0, 2, (n,), generator=g)
            q[torch.arange(n), ax] = bb[ax, side] + (torch.rand(n, generator=g, dtype=F64) * 2 - 1) * 6e-3
        return _src_of(q, pose), pose, bound
    else:
        Rs, Rd = _rot(rs), _rot(rs)
        ts = torch.tensor(rs.uniform(-1, 1, 3), dtype=F32)
        td = torch.tensor(rs.uniform(-1, 1, 3), dtype=F32)
        pose = _pose(Rs, ts, Rd, td)
    if kind == "slack":
        # vertices 1e-4, 1e-3 and 3e-3 m either side of a face, under a generic rotation
        q = (torch.rand(n, 3, generator=g, dtype=F64) * 0.9 + 0.05) * (b[:, 1] - b[:, 0]) + b[:, 0]
        ax = torch.randint(0, 3, (n,), generator=g)
        side = torch.randint(0, 2, (n,), generator=g)
        dist = torch.tensor([1e-4, 1e-3, 3e-3], dtype=F64)[torch.randint(0, 3, (n,), generator=g)]
        sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
        face = b[ax, side]
        q[torch.arange(n), ax] = face + sign * dist
        return _src_of(q, pose), pose, BOUND
    q = (torch.rand(n, 3, generator=g, dtype=F64) * 1.3 - 0.15) * (b[:, 1] - b[:, 0]) + b[:, 0]
    return _src_of(q, pose), pose, BOUND


def _kernel(p, fsrc, fdev, bound, pose, lt, ignore_mask=0):
    bnd = [bound[a][0] for a in range(3)] + [bound[a][1] for a in range(3)]
    fsd = fsrc if fsrc.is_cuda else fsrc.to(DEV)
    return torch.ops.miso.pair_latent_fwd_bwd(pose.to(DEV), p.to(DEV), fsd, fdev, bnd, ignore_mask, 0,
                                              {"L1": 1, "L2": 2}[lt]).cpu()


def _run_pair(layout, nlev, n, lt, kind, seed, ignore_mask=0, ld_extra=3):
    import miso_amd.torch_ops  # noqa: F401  (registers torch.ops.miso)
    g = torch.Generator().manual_seed(seed)
    rs = np.random.RandomState(seed)
    p, pose, bound = _geometry(kind, n, g, rs)
    xyz = [(8, 4, 4), (16, 8, 8)] if kind == "perm" else LEVEL_XYZ
    fcpu, fdev = _levels(layout, nlev, g, xyz)
    F_ = sum(f.shape[1] for f in fcpu)
    full = torch.randn(n, F_ + ld_extra, generator=g) * 0.1            # source rows with ld > F
    fsrc = full[:, :F_]
    fsd = full.to(DEV)[:, :F_]
    assert fsd.stride(0) == F_ + ld_extra
    got = _kernel(p, fsd, fdev, bound, pose, lt, ignore_mask)
    sums, A = R.pair_latent_sums64(p, fsrc, fcpu, bound, pose, lt, ignore_mask)
    _check_sums(f"{layout} L{nlev} n={n} {lt} {kind}", got, sums, A)
    return got, sums


# --------------------------------------------------------------------------- #
# miso_pair_latent: one pair
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 100003])
def test_pair_sums_batch_sizes(n):
    got, sums = _run_pair("cl4", 2, n, "L2" if n % 2 else "L1", "generic", 100 + n)
    if n == 0:
        assert got.abs().max().item() == 0.0


@pytest.mark.parametrize("layout", ["cl4", "cl8", "nc4", "nc3", "nc1"])
@pytest.mark.parametrize("nlev", [1, 2, 3])
@pytest.mark.parametrize("lt", ["L2", "L1"])
def test_pair_sums_layouts_and_levels(layout, nlev, lt):
    _run_pair(layout, nlev, 3001, lt, "generic", 7 * nlev + len(layout))


@pytest.mark.parametrize("layout", ["cl4", "nc3"])
def test_pair_sums_with_an_ignored_level(layout):
    _run_pair(layout, 3, 3001, "L2", "generic", 41, ignore_mask=0b010)


@pytest.mark.parametrize("kind", ["perm", "slack", "far_t", "far_p", "far_p4"])
@pytest.mark.parametrize("lt", ["L2", "L1"])
def test_pair_sums_geometry(kind, lt):
    """inclusive faces and floor cells (perm), the slack band of the pass-1 filter (slack), large |t| and large |p|"""
    got, sums = _run_pair("cl4", 2, 6007, lt, kind, 53)
    assert sums[1] > 100


@pytest.mark.parametrize("kind", ["far_p_band", "far_p4_band"])
def test_slack_band_far_from_the_origin(kind):
    """Vertices within 6e-3 m of the faces of a bound 1e3 / 1e4 m from the origin (|p| ~ |q|, small |t|): the pass-1
    filter of the pair kernels (the composed map M p + q0 against the bound widened / shrunk by the slack) must leave
    every decision the exact test would change to the exact test.  Counts exactly the src_to_dst32 count in
    miso_pair_latent, in the batched kernel (with the box cull) and in ops.overlap_count."""
    from miso_amd import ops
    got, sums = _run_pair("cl4", 2, 30011, "L2", kind, 59)
    assert 1000 < sums[1] < 29000
    g = torch.Generator().manual_seed(59)
    rs = np.random.RandomState(59)
    p, pose, bound = _geometry(kind, 30011, g, rs)
    _, _, m = R.src_to_dst32(p, pose[:9], pose[9:12], pose[12:21], pose[21:24], bound)
    Rs, ts, Rd, td = pose[:9].view(3, 3), pose[9:12].view(3, 1), pose[12:21].view(3, 3), pose[21:24].view(3, 1)
    cnt = ops.overlap_count(Rs.to(DEV), ts.to(DEV), Rd.to(DEV), td.to(DEV), p.to(DEV), torch.tensor(bound))
    assert int(cnt.item()) == int(m.sum())
    fcpu, fdev = _levels("cl4", 1, g)
    fsrc = torch.randn(p.shape[0], 4, generator=g) * 0.1
    meta = ops.GridMeta(tuple(b[0] for b in bound), tuple(b[1] for b in bound))
    d = dict(src=0, dst=1, coords=p.to(DEV), feats_src=fsrc.to(DEV), feats_dst=fdev, meta_dst=meta, gate_pts=None)
    plan = ops.AlignPlan(torch.stack([Rs, Rd]).to(DEV), torch.stack([ts, td]).to(DEV), [d], cull=True)
    plan.params.zero_()
    plan.iteration_a()
    assert torch.equal(plan.poses.cpu(), torch.stack([pose[:12], pose[12:]]))
    s2, A2 = R.pair_latent_sums64(p, fsrc, fcpu, bound, pose, "L2")
    _check_sums(f"AlignPlan {kind}", plan.pair_out.cpu()[0], s2, A2)


def test_pair_sums_l1_zero_residual():
    """L1 with a constant destination level and f_src equal to it: interior residuals are exactly 0 (inv_norm = 0)"""
    import miso_amd.torch_ops  # noqa: F401
    g = torch.Generator().manual_seed(3)
    rs = np.random.RandomState(3)
    p, pose, bound = _geometry("generic", 4001, g, rs)
    fcpu, fdev = _levels("cl4", 1, g, const=0.25)
    fsrc = torch.full((4001, 4), 0.25)
    got = _kernel(p, fsrc, fdev, bound, pose, "L1")
    sums, A = R.pair_latent_sums64(p, fsrc, fcpu, bound, pose, "L1")
    assert torch.isfinite(got).all()
    _check_sums("L1 zero residual", got, sums, A)


def test_pair_sums_nonfinite_vertices_and_pose():
    import miso_amd.torch_ops  # noqa: F401
    g = torch.Generator().manual_seed(4)
    rs = np.random.RandomState(4)
    n = 5003
    p, pose, bound = _geometry("generic", n, g, rs)
    sel = torch.randperm(n, generator=g)[:300]
    p[sel[:100], 0] = float("nan")
    p[sel[100:200], 1] = float("inf")
    p[sel[200:], 2] = -float("inf")
    fcpu, fdev = _levels("cl4", 2, g)
    fsrc = torch.randn(n, 8, generator=g) * 0.1
    got = _kernel(p, fsrc, fdev, bound, pose, "L2")
    sums, A = R.pair_latent_sums64(p, fsrc, fcpu, bound, pose, "L2")
    _check_sums("non-finite vertices", got, sums, A)
    from miso_amd import ops
    bad = pose.clone()
    bad[3] = float("nan")                                   # a NaN in R_s
    got = _kernel(p, fsrc, fdev, bound, bad, "L2")
    assert got.abs().max().item() == 0.0
    meta = ops.GridMeta(tuple(b[0] for b in bound), tuple(b[1] for b in bound))
    val = ops.pair_latent(bad[:9].view(3, 3).to(DEV), bad[9:12].view(3, 1).to(DEV), bad[12:21].view(3, 3).to(DEV),
                          bad[21:24].view(3, 1).to(DEV), p.to(DEV), fsrc.to(DEV), fdev, meta, "L2")
    assert val.item() == 0.0


# --------------------------------------------------------------------------- #
# ops level: ops.pair_latent and pair_latent_multi against the fp64 chain rule on fp64 sums
# --------------------------------------------------------------------------- #
def _grad_bars(sums, A, pose, lt, n_ch):
    denom = max(float(sums[1]), 1.0) * (n_ch if lt == "L2" else 1)
    hA = (pose[12:21].double().view(3, 3).abs() @ A[2:5]).view(3, 1) / denom
    return (A[0] / denom, A[14:23].view(3, 3) / denom, hA, A[5:14].view(3, 3) / denom, hA)


@pytest.mark.parametrize("lt", ["L2", "L1"])
def test_ops_pair_latent_and_multi_vs_fp64_chain_rule(lt):
    from miso_amd import ops
    g = torch.Generator().manual_seed(61)
    rs = np.random.RandomState(61)
    p, pose, bound = _geometry("generic", 20011, g, rs)
    fcpu, fdev = _levels("cl4", 2, g)
    fsrc = torch.randn(p.shape[0], 8, generator=g) * 0.1
    sums, A = R.pair_latent_sums64(p, fsrc, fcpu, bound, pose, lt)
    want = R.pair_pose_grads64(sums, pose[12:21], lt, 8)
    bars = _grad_bars(sums, A, pose, lt, 8)
    meta = ops.GridMeta(tuple(b[0] for b in bound), tuple(b[1] for b in bound))
    ps = [pose[:9].view(3, 3), pose[9:12].view(3, 1), pose[12:21].view(3, 3), pose[21:24].view(3, 1)]
    pd = [t.clone().to(DEV).requires_grad_(True) for t in ps]
    val = ops.pair_latent(*pd, p.to(DEV), fsrc.to(DEV), fdev, meta, lt)
    gg = torch.autograd.grad(val, pd)
    for name, got, ref, bar in zip(("loss", "R_s", "t_s", "R_d", "t_d"), (val,) + gg, want, bars):
        got = got.detach().double().cpu()
        # + one fp32 rounding of the returned value
        assert ((got - ref).abs() <= REL * bar + 2 ** -23 * ref.abs() + 1e-12).all(), (name, got, ref, bar)
    # pair_latent_multi: submaps 0 and 1, pairs (0, 1) and (1, 0) on the same data
    R_all = torch.stack([ps[0], ps[2]]).to(DEV).requires_grad_(True)
    t_all = torch.stack([ps[1], ps[3]]).to(DEV).requires_grad_(True)
    grid = ops._fill_grid(fdev, meta)
    plan = dict(pairs=[(0, 1), (1, 0)], coords=[p.to(DEV)] * 2, feats_src=[fsrc.to(DEV)] * 2, grids=[grid, grid],
                n_ch=[8, 8], loss_type=lt, gate_pts=None, overlap_thresh=0.0)
    sw = torch.cat([pose[12:], pose[:12]])                  # the pose vector of pair (1, 0)
    sums2, A2 = R.pair_latent_sums64(p, fsrc, fcpu, bound, sw, lt)
    losses = ops.pair_latent_multi(R_all, t_all, plan)
    gR, gt = torch.autograd.grad(losses.sum(), (R_all, t_all))
    w2 = R.pair_pose_grads64(sums2, sw[12:21], lt, 8)
    b2 = _grad_bars(sums2, A2, sw, lt, 8)
    want_R = [want[1] + w2[3], want[3] + w2[1]]
    want_t = [want[2] + w2[4], want[4] + w2[2]]
    bar_R = [bars[1] + b2[3], bars[3] + b2[1]]
    bar_t = [bars[2] + b2[4], bars[4] + b2[2]]
    for s in range(2):
        for got, ref, bar in ((gR[s], want_R[s], bar_R[s]), (gt[s], want_t[s], bar_t[s])):
            got = got.double().cpu()
            assert ((got - ref).abs() <= REL * bar + 2 ** -23 * ref.abs() + 1e-12).all(), (s, got, ref, bar)


# --------------------------------------------------------------------------- #
# AlignPlan: the batched pair kernels, epilogue A and B
# --------------------------------------------------------------------------- #
DR2 = [0.0, 1e-6, 2.5e-5, 4e-4, 0.09, 2.25]           # |dr|^2 of the corrections: 4x or more from the clamp at 1e-4


def _lattice(nx, ny, nz, bound):
    b = torch.tensor(bound, dtype=F32)
    ax = [torch.linspace(float(b[a, 0]), float(b[a, 1]), m) for a, m in enumerate((nx, ny, nz))]
    zz, yy, xx = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return torch.stack([xx.flatten(), yy.flatten(), zz.flatten()], 1).contiguous(), (nx, ny, nz)


def _submaps(S, seed, dr2=None, spread=1.5):
    rs = np.random.RandomState(seed)
    R0 = torch.stack([_rot(rs, 0.3) for _ in range(S)])
    t0 = torch.tensor(rs.uniform(-spread, spread, (S, 3, 1)), dtype=F32)
    prm = torch.zeros(S, 6)
    for s in range(S):
        v = rs.standard_normal(3)
        r2 = dr2[s % len(dr2)] if dr2 is not None else rs.uniform(0, 0.01)
        prm[s, :3] = torch.tensor(v / np.linalg.norm(v) * math.sqrt(r2), dtype=F32)
        prm[s, 3:] = torch.tensor(rs.uniform(-0.05, 0.05, 3), dtype=F32)
    return R0, t0, prm


def _plan_pairs(S, pair_list, n, seed, gate, nlev=2, shared=False):
    """AlignPlan pair dicts plus the CPU copies the oracle needs.  gate: None | "points" | "lattice"."""
    from miso_amd import ops
    g = torch.Generator().manual_seed(seed)
    meta = ops.GridMeta(tuple(b[0] for b in BOUND), tuple(b[1] for b in BOUND))
    b = torch.tensor(BOUND)
    cache = {}

    def per_submap(s):
        key = 0 if shared else s
        if key not in cache:
            fcpu, fdev = _levels("cl4", nlev, g)
            p = (torch.rand(n, 3, generator=g) * 1.2 - 0.1) * (b[:, 1] - b[:, 0]) + b[:, 0]
            full = torch.randn(n, 4 * nlev + 3, generator=g) * 0.1          # ld > F
            fsrc = full[:, :4 * nlev]
            gp, dims = _lattice(9, 7, 8, BOUND)
            cache[key] = dict(fcpu=fcpu, fdev=fdev, p=p, pd=p.to(DEV), fsrc=fsrc, fsd=full.to(DEV)[:, :4 * nlev], gp=gp,
                              gpd=gp.to(DEV), dims=dims)
        return cache[key]

    dicts, host = [], []
    for a, c in pair_list:
        sa, sc = per_submap(a), per_submap(c)
        d = dict(src=a, dst=c, coords=sa["pd"], feats_src=sa["fsd"], feats_dst=sc["fdev"], meta_dst=meta,
                 gate_pts=sa["gpd"] if gate else None)
        if gate == "lattice":
            d["gate_dims"] = sa["dims"]
        dicts.append(d)
        host.append(dict(src=a, dst=c, p=sa["p"], fsrc=sa["fsrc"], fdst=sc["fcpu"], gp=sa["gp"], n_ch=4 * nlev,
                         gate_n=sa["gp"].shape[0] if gate else 0))
    return dicts, host


def _params(plan):
    """(S,6) corrections, read without the `params` property (which makes the next iteration_a run its own prologue
    instead of taking the poses epilogue B left)"""
    return plan._view(0, 6 * plan.S).view(plan.S, 6).cpu().clone()


def _check_plan_iteration(plan, host, S, R0, lt, thresh, memo=None):
    """pair_out, overlap counts and flat of the last iteration_a against the oracles, at plan.poses"""
    poses = plan.poses.cpu()
    params = _params(plan)
    out = plan.pair_out.cpu()
    cnt = plan.overlap_counts.cpu()
    sums_all, A_all = torch.zeros(len(host), 24, dtype=F64), torch.zeros(len(host), 24, dtype=F64)
    for i, h in enumerate(host):
        pose = torch.cat([poses[h["src"]], poses[h["dst"]]])
        key = (id(h["p"]), id(h["fdst"][0]), tuple(pose.tolist()))
        if memo is not None and key in memo:
            sums, A = memo[key]
        else:
            sums, A = R.pair_latent_sums64(h["p"], h["fsrc"], h["fdst"], BOUND, pose, lt)
            if memo is not None:
                memo[key] = (sums, A)
        _check_sums(f"pair {i} ({h['src']},{h['dst']})", out[i], sums, A)
        sums_all[i], A_all[i] = sums, A
        if h["gate_n"]:
            _, _, m = R.src_to_dst32(h["gp"], pose[:9], pose[9:12], pose[12:21], pose[21:24], BOUND)
            assert int(cnt[i].item()) == int(m.sum()), (i, cnt[i].item(), int(m.sum()))
    # epilogue A fed the kernel's own sums: 1e-6 of the absolute-value pull-back (+ the fp32 store)
    losses, flat, absf = R.align_epilogue64(out, cnt, host, S, poses, R0, params, loss_type=lt, overlap_thresh=thresh)
    got = plan.flat_reduce.cpu().double()
    assert torch.equal(got[6 * S + 1:], flat[6 * S + 1:]), "had-a-gradient flags"
    err = (got[:6 * S] - flat[:6 * S]).abs()
    assert (err <= 1e-6 * absf + 2 ** -23 * flat[:6 * S].abs() + 1e-12).all(), (err, absf)
    # (the loss sum: P fp32 additions of non-negative pair losses)
    assert abs(got[6 * S].item() - flat[6 * S].item()) <= len(host) * 2 ** -24 * flat[6 * S].abs().item() + 1e-12
    torch.testing.assert_close(plan.pair_losses.cpu().double(), losses, rtol=2e-7, atol=0)
    # against the full fp64 oracle: the per-sum bounds pushed through the same absolute-value map
    _, flat64, absf64 = R.align_epilogue64(sums_all, cnt, host, S, poses, R0, params, loss_type=lt,
                                           overlap_thresh=thresh)
    bound_out = A_all.clone()
    bound_out[:, 1] = sums_all[:, 1]
    _, _, absA = R.align_epilogue64(bound_out, cnt, host, S, poses, R0, params, loss_type=lt, overlap_thresh=thresh)
    err = (got[:6 * S] - flat64[:6 * S]).abs()
    assert (err <= REL * absA + 1e-6 * absf64 + 2 ** -23 * flat64[:6 * S].abs() + 1e-12).all(), (err, absA)
    return got


@pytest.mark.parametrize("gate", [None, "points", "lattice"])
@pytest.mark.parametrize("cull", [True, False])
def test_align_plan_two_iterations(gate, cull):
    """S = 6, all 30 ordered pairs (gate on: pair_stage_kernel; gate off: pair_latent_batch_kernel), the six |dr|^2 of
    DR2, two iterations -- the second in the launch order epilogue A ranked -- with epilogue B against fp64 and the
    regulariser just below and above its thresholds."""
    from miso_amd import ops
    S, lt, thresh = 6, "L2" if cull else "L1", 0.05
    R0, t0, prm = _submaps(S, 17, DR2)
    rad, tm = 0.25, 0.04
    # the regulariser: submap 2 just below, 3 just above the rotation threshold; 4 just above the translation one
    prm[2, :3] *= (rad * (1 - 1e-3)) / prm[2, :3].norm()
    prm[3, :3] *= (rad * (1 + 1e-3)) / prm[3, :3].norm()
    prm[4, 3:] *= (tm * (1 + 1e-3)) / prm[4, 3:].norm()
    pairs = [(a, c) for a in range(S) for c in range(S) if a != c]
    dicts, host = _plan_pairs(S, pairs, 2503, 5, gate)
    kw = dict(loss_type=lt, align_weight=3000.0, overlap_thresh=thresh, lr=1e-2, reg_weight=2.0,
              reg_thresh_rad=rad, reg_thresh_m=tm, ring_iters=2, cull=cull)
    plan = ops.AlignPlan(R0.to(DEV), t0.to(DEV), dicts, **kw)
    plan.params.copy_(prm.to(DEV))
    m = torch.zeros(S, 6, dtype=F64)
    v = torch.zeros(S, 6, dtype=F64)
    steps = torch.zeros(S, dtype=torch.int64)
    for it in range(2):
        plan.iteration_a()
        before = _params(plan)
        flat = _check_plan_iteration(plan, host, S, R0, lt, thresh)
        m_k = plan._view(6, 6 * S).cpu().view(S, 6).double()
        v_k = plan._view(7, 6 * S).cpu().view(S, 6).double()
        plan.iteration_b()
        total, prm64, m64, v64, t64 = R.align_epilogue_b64(flat, before, m_k if it else m, v_k if it else v, steps,
                                                           lr=1e-2, reg_weight=2.0, reg_thresh_rad=rad,
                                                           reg_thresh_m=tm)
        steps = t64
        after = _params(plan).double()
        assert torch.equal(plan.adam_steps.cpu().to(torch.int64), t64)
        torch.testing.assert_close(after, prm64, rtol=0, atol=1e-7 + 1e-6 * 1e-2)
        torch.testing.assert_close(plan._view(6, 6 * S).cpu().view(S, 6).double(), m64, rtol=2e-6, atol=1e-12)
        torch.testing.assert_close(plan._view(7, 6 * S).cpu().view(S, 6).double(), v64, rtol=2e-6, atol=1e-18)
        assert abs(plan.ring()[it, 0].item() - total) <= 1e-6 * abs(total)


def test_align_plan_nan_guard():
    """A NaN correction makes the regulariser, and so the iteration's loss, NaN: epilogue B skips the step (base.py:
    147-151) -- every value, moment and step count stays, as align_epilogue_b64 restates -- and counts it.  The NaN
    submap's pairs have all-zero sums (no vertex is in bound under a NaN pose)."""
    from miso_amd import ops
    S = 4
    R0, t0, prm = _submaps(S, 43)
    prm[2, 1] = float("nan")
    pairs = [(a, c) for a in range(S) for c in range(S) if a != c]
    dicts, host = _plan_pairs(S, pairs, 1501, 47, None)
    plan = ops.AlignPlan(R0.to(DEV), t0.to(DEV), dicts, loss_type="L2", reg_weight=2.0, reg_thresh_rad=0.1,
                         reg_thresh_m=0.1, ring_iters=1)
    plan.params.copy_(prm.to(DEV))
    plan.iteration_a()
    out = plan.pair_out.cpu()
    for i, (a, c) in enumerate(pairs):
        if 2 in (a, c):
            assert out[i].abs().max().item() == 0.0, (a, c)
    flat = plan.flat_reduce.cpu().double()
    m0, v0 = plan._view(6, 6 * S).cpu().view(S, 6).double(), plan._view(7, 6 * S).cpu().view(S, 6).double()
    steps0 = plan.adam_steps.cpu().to(torch.int64)
    plan.iteration_b()
    total, prm64, m64, v64, t64 = R.align_epilogue_b64(flat, prm, m0, v0, steps0, reg_weight=2.0, reg_thresh_rad=0.1,
                                                       reg_thresh_m=0.1)
    assert math.isnan(total) and math.isnan(plan.ring()[0, 0].item())
    assert torch.allclose(_params(plan).double(), prm64, rtol=0, atol=0, equal_nan=True)
    assert torch.equal(plan._view(6, 6 * S).cpu().view(S, 6).double(), m64)
    assert torch.equal(plan._view(7, 6 * S).cpu().view(S, 6).double(), v64)
    assert torch.equal(plan.adam_steps.cpu().to(torch.int64), t64)
    assert plan.ctrl() == dict(steps=0, stopped=False, iterations=1, skipped=1)


def test_align_plan_multi_trip_56_pairs():
    """S = 8 and all 56 ordered pairs on one coordinate tensor, one set of grids and one set of poses: 7168 / 56 = 128
    workgroups per pair, so 600 000 vertices take three trips of every workgroup (the LDS list reused, the pair stage
    striding by pair_blocks).  One oracle evaluation serves all pairs; gate off and gate on (point list)."""
    from miso_amd import ops
    S, lt = 8, "L2"
    rs = np.random.RandomState(8)
    R1 = _rot(rs, 0.3)
    R0 = R1.expand(S, 3, 3).contiguous()
    t0 = torch.tensor([[0.2], [-0.1], [0.3]]).expand(S, 3, 1).contiguous()
    pairs = [(a, c) for a in range(S) for c in range(S) if a != c]
    memo = {}
    dicts_on, host_on = _plan_pairs(S, pairs, 600000, 9, "points", shared=True)
    dicts_off = [dict(d, gate_pts=None) for d in dicts_on]
    host_off = [dict(h, gate_n=0) for h in host_on]
    for dicts, host in ((dicts_off, host_off), (dicts_on, host_on)):
        plan = ops.AlignPlan(R0.to(DEV), t0.to(DEV), dicts, loss_type=lt, overlap_thresh=0.01)
        plan.params.zero_()
        plan.iteration_a()
        _check_plan_iteration(plan, host, S, R0, lt, 0.01, memo)


def test_align_plan_190_pairs_some_gated_off():
    """S = 20, 190 distinct pairs (P > 128: epilogue A stages pairs in two passes, no launch reordering), about
    2 000 vertices each, spread so that some pairs fail the overlap gate."""
    from miso_amd import ops
    S, lt, thresh = 20, "L2", 0.2
    R0, t0, prm = _submaps(S, 23, spread=4.0)
    pairs = [(a, c) for a in range(S) for c in range(a + 1, S)]
    dicts, host = _plan_pairs(S, pairs, 2011, 29, "points")
    plan = ops.AlignPlan(R0.to(DEV), t0.to(DEV), dicts, loss_type=lt, overlap_thresh=thresh)
    plan.params.copy_(prm.to(DEV))
    plan.iteration_a()
    _check_plan_iteration(plan, host, S, R0, lt, thresh)
    frac = plan.overlap_counts.cpu() / 9 / 7 / 8
    assert (frac <= thresh).any() and (frac > thresh).any()


def test_align_plan_64_submaps():
    """S = 64 (every thread of epilogue A's 256 owns a quarter of a submap), 63 pairs"""
    from miso_amd import ops
    S, lt = 64, "L1"
    R0, t0, prm = _submaps(S, 31, DR2, spread=0.5)
    pairs = [(s, s + 1) for s in range(S - 1)]
    dicts, host = _plan_pairs(S, pairs, 701, 37, "lattice", nlev=1)
    plan = ops.AlignPlan(R0.to(DEV), t0.to(DEV), dicts, loss_type=lt, overlap_thresh=0.01)
    plan.params.copy_(prm.to(DEV))
    plan.iteration_a()
    _check_plan_iteration(plan, host, S, R0, lt, 0.01)


# --------------------------------------------------------------------------- #
# Overlap counts: exactly the kernel arithmetic's count
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("angle", [0.4, 3e-3])
def test_overlap_counts_exact(angle):
    """ops.overlap_count and AlignPlan.overlap_counts (lattice and point-list gates) equal the src_to_dst32 count,
    also with faces met at a shallow angle (two submaps a fraction of a degree apart)."""
    from miso_amd import ops
    rs = np.random.RandomState(int(angle * 1000) + 1)
    gp, dims = _lattice(161, 97, 113, BOUND)
    Rs = torch.eye(3)
    Rd = torch.tensor(gc.rodrigues(rs.standard_normal(3) / math.sqrt(3) * angle), dtype=F32)
    ts = torch.zeros(3)
    td = torch.tensor([0.51, -0.37, 0.23])
    _, _, m = R.src_to_dst32(gp, Rs, ts, Rd, td, BOUND)
    want = int(m.sum())
    got = ops.overlap_count(Rs.to(DEV), ts.view(3, 1).to(DEV), Rd.to(DEV), td.view(3, 1).to(DEV), gp.to(DEV),
                            torch.tensor(BOUND))
    assert int(got.item()) == want
    R0 = torch.stack([Rs, Rd])
    t0 = torch.stack([ts.view(3, 1), td.view(3, 1)])
    fcpu, fdev = _levels("cl4", 1, torch.Generator().manual_seed(1))
    meta = ops.GridMeta(tuple(b[0] for b in BOUND), tuple(b[1] for b in BOUND))
    x = gp[:1000].to(DEV)
    for lattice in (False, True):
        d = dict(src=0, dst=1, coords=x, feats_src=torch.zeros(1000, 4, device=DEV), feats_dst=fdev, meta_dst=meta,
                 gate_pts=gp.to(DEV))
        if lattice:
            d["gate_dims"] = dims
        plan = ops.AlignPlan(R0.to(DEV), t0.to(DEV), [d])
        plan.params.zero_()
        plan.iteration_a()
        pz = plan.poses.cpu()
        assert torch.equal(pz[0], torch.cat([Rs.flatten(), ts])) and torch.equal(pz[1], torch.cat([Rd.flatten(), td]))
        assert int(plan.overlap_counts.cpu()[0].item()) == want, (lattice, plan.overlap_counts.cpu()[0].item(), want)


