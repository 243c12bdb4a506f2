"""Inputs and float64 oracles of MIPS-Fusion's projected-match residual (csrc/pair_sdf.hip, kinds 1 and 2;
ops.AlignPlan(residual="mips"); grid_opt/align/mips.py), shared by test_mips_host.py (no GPU) and test_mips.py.

Two statements of the same loss:

mips_literal64   the reference's formula written out: q = R_d^T (R_s p + t_s - t_d), s = s_dst(q), g = grad_q s detached,
                 match_dst = q - s g, match_src = R_s^T (R_d match_dst + t_d - t_s), cons = (p - match_src) . n or
                 p - match_src, loss = weight mean(cons^2), with R = R0 Exp(dr) (miso_amd/so3.py), t = t0 + dt in float64
                 and autograd to (dr_s, dt_s, dr_d, dt_d).
mips_sums64      the closed form the kernel sums.  p - match_src = s M^T g with M = R_d^T R_s, so
                   plane   a = g . (M n); term (s a)^2; cotangent to q 2 s a^2 g; S2 = sum 2 s^2 a g (x) n, which adds
                           R_s S2^T to d / d R_d and R_d S2 to d / d R_s;
                   point   term s^2 |g|^2; cotangent to q 2 s |g|^2 g; the mean is over 3 count elements.
                 Its 24 numbers are miso_pair_latent's: [0] sum term, [1] count, [2:5] sum cotangent, [5:14] d / d R_d,
                 [14:23] d / d R_s.  Beside them the absolute-value yardstick A, built like pair_sdf_cases.pair_sdf_sums64's
                 with |s|, |g|, |n| and |M| componentwise in every product.

pull_back maps the 24 sums to d loss / d (dr, dt) of both submaps the way align_epilogue_a_kernel does, in float64, and
maps A the same way with every matrix entry in absolute value."""
import functools

import torch

import pair_sdf_cases as pc
from oracle import ref_torch as R

F32, F64 = torch.float32, torch.float64
GRIDS = ("c4l2", "c8l1")
CONSTRAINTS = ("point_to_plane", "point_to_point")
N_CH = {"point_to_plane": 1, "point_to_point": 3}
BOUND = pc.BOUND

# The bar on the raw sums: |got - fp64| <= REL_MIPS A + 1e-12.  Set from the dtype=F32 restatement of mips_sums64 against
# float64 on every case of the tests (grid x n in {2049, 130} x constraint, on the CPU): worst (|fp32 - fp64| - 1e-12) / A
#   point_to_plane  c4l2 8.6e-8 (n 2049) 1.9e-7 (n 130)   c8l1 4.0e-8 / 1.5e-7
#   point_to_point  c4l2 5.0e-7 / 5.0e-7                   c8l1 1.7e-7 / 4.5e-7
# 4 x 4.96e-7 = 1.98e-6, rounded up to one digit.  (test_mips_host.py::test_fp32_restatement_is_within_the_bar prints
# the ratios.)  pair_sdf_cases.REL, for one gradient factor, is 1e-4: the cap of 1e-3 is far away.
REL_MIPS = 2e-6

# The surface threshold of the loop tests on golden_cases.atlas_sdf_batch (gt sdf ~ N(0, 0.1), 900 rows): at the reference's
# 1e-3 a handful of rows are surface.  0.05 keeps 111 / 96 / 127 rows of submaps 0 / 1 / 2 but only 12 of pair (0, 2) and
# 10 of (2, 0) in the destination's bound at the initial poses; 0.08 is the first of 0.05, 0.06, 0.07, 0.08 at which every
# ordered pair holds 16 or more: surface rows 166 / 161 / 203, in bound (0,1) 54, (0,2) 16, (1,0) 63, (1,2) 63, (2,0) 17,
# (2,1) 65 (test_mips_host.py::test_atlas_case_counts asserts it).
SURF = 0.08


@functools.lru_cache(maxsize=None)
def case(grid, n, seed=0):
    """pair_sdf_cases.case (destination levels, decoder, pose, safe rows) plus unit source normals (n,3) fp32."""
    c = dict(pc.case(grid, n, seed))
    g = torch.Generator().manual_seed(900 + 13 * seed + n)
    v = torch.randn(n, 3, generator=g)
    c["normals"] = (v / v.norm(dim=1, keepdim=True).clamp(min=1e-12)).to(F32)
    return c


def _total(x, dtype):
    """sum over rows: float64, or a kernel lane's way -- runs of 8 rows in fp32, then float64"""
    x = x.reshape(x.shape[0], -1)
    if dtype == F64:
        return x.double().sum(0)
    pad = (-x.shape[0]) % 8
    x = torch.cat([x, x.new_zeros(pad, x.shape[1])]).view(-1, 8, x.shape[1])
    return x.sum(1).double().sum(0)


def mips_sums64(p, normals, feats_dst, bound, pose, ws, bs, constraint, dtype=F64, map64=False, s2=True, g_sign=None):
    """(sums (24,), A (24,)) float64 -- module docstring.  The in-bound set and q are R.src_to_dst32's on the fp32 pose
    (the kernel's own map); map64: ``pose`` is float64 and is used as it is, the map and the bound test in float64 (the
    closed form against the literal formula at exactly orthonormal rotations).  dtype F32: what a careful fp32
    implementation computes at the same q -- decoder, gradient, M, the terms in fp32, runs of 8 rows summed in fp32, then
    float64, S and S2 folded with the poses in float64 as the kernel's tail does.  s2=False leaves the S2 term out and
    g_sign (n,) of +-1 flips g on rows: the two mistakes the bar must see."""
    assert constraint in CONSTRAINTS
    sums, A = torch.zeros(24, dtype=F64), torch.zeros(24, dtype=F64)
    if p.shape[0] == 0:
        return sums, A
    if map64:
        pose = torch.as_tensor(pose, dtype=F64).reshape(24)
        Rs, ts, Rd, td = pose[:9].view(3, 3), pose[9:12], pose[12:21].view(3, 3), pose[21:24]
        b64 = torch.as_tensor(bound, dtype=F64)
        q = (p.double() @ Rs.T + (ts - td)) @ Rd
        m = ((q >= b64[:, 0]) & (q <= b64[:, 1])).all(1)
    else:
        pose = torch.as_tensor(pose, dtype=F32).reshape(24)
        Rs, ts, Rd, td = pose[:9].view(3, 3), pose[9:12], pose[12:21].view(3, 3), pose[21:24]
        _, q, m = R.src_to_dst32(p, Rs, ts, Rd, td, bound)
    idx = torch.nonzero(m).flatten()
    sums[1] = float(idx.numel())
    if idx.numel() == 0:
        return sums, A
    b = torch.as_tensor(bound, dtype=F64 if map64 else F32).to(dtype)
    qi = q[idx].to(dtype).requires_grad_(True)
    s = R.sdf_gather([f.to(dtype) for f in feats_dst], b, qi, [w.to(dtype) for w in ws],
                     [None if v is None else v.to(dtype) for v in bs])[:, 0]
    (g,) = torch.autograd.grad(s.sum(), qi)
    s = s.detach()
    if g_sign is not None:
        g = g * g_sign[idx].to(dtype)[:, None]
    pi = p[idx]
    nv = torch.as_tensor(normals, dtype=F32)[idx].to(dtype)
    M = Rd.to(dtype).T @ Rs.to(dtype)
    sa, ga, na = s.abs().double(), g.abs().double(), nv.abs().double()
    S2 = S2a = torch.zeros(3, 3, dtype=F64)
    if constraint == "point_to_plane":
        a = (g * (nv @ M.T)).sum(1)
        c = s * a
        term, gq = c * c, (2 * (c * a))[:, None] * g
        aa = (ga * (na @ M.abs().double().T)).sum(1)
        term_a, gq_a = (sa * aa) ** 2, (2 * sa * aa * aa)[:, None] * ga
        if s2:
            S2 = _total(((2 * (s * c))[:, None] * g)[:, :, None] * nv[:, None, :], dtype).view(3, 3)
        S2a = (((2 * sa * sa * aa)[:, None] * ga)[:, :, None] * na[:, None, :]).sum(0)
    else:
        g2 = (g * g).sum(1)
        sg = s * g2
        term, gq = s * sg, (2 * sg)[:, None] * g
        term_a, gq_a = term.abs().double(), gq.abs().double()
    Rs64, ts64, Rd64, td64, p64 = Rs.double(), ts.double(), Rd.double(), td.double(), pi.double()
    G = _total(gq, dtype)
    sums[0], sums[2:5] = _total(term, dtype)[0], G
    # S = sum p (x) gq, then the kernel's tail: Rs S + (ts - td) G [+ Rs S2^T] and Rd S^T [+ Rd S2]
    S = _total((pi.to(dtype) if dtype == F32 else p64)[:, :, None] * gq[:, None, :], dtype).view(3, 3)
    sums[5:14] = (Rs64 @ S + (ts64 - td64)[:, None] * G[None, :] + Rs64 @ S2.T).flatten()
    sums[14:23] = (Rd64 @ S.T + Rd64 @ S2).flatten()
    dabs = p64.abs() @ Rs64.abs().T + (ts64 - td64).abs()
    A[0], A[2:5] = term_a.sum(), gq_a.sum(0)
    A[5:14] = ((dabs[:, :, None] * gq_a[:, None, :]).sum(0) + Rs64.abs() @ S2a.T).flatten()
    A[14:23] = (((gq_a @ Rd64.abs().T)[:, :, None] * p64.abs()[:, None, :]).sum(0) + Rd64.abs() @ S2a).flatten()
    return sums, A


def excess(got, sums, A):
    """R.pair_sums_excess at REL_MIPS: count exact, the others |got - fp64| <= REL_MIPS A + 1e-12."""
    return R.pair_sums_excess(got, sums, A, rel=REL_MIPS)


def _exp_jacobian64(w):
    """d Exp(w)_ij / d w_k (3,3,3), float64, through miso_amd/so3.py"""
    from miso_amd import so3
    w = torch.as_tensor(w, dtype=F64).reshape(3)
    return torch.autograd.functional.jacobian(lambda v: so3.so3_exp_map(v.view(1, 3))[0], w)


def pull_back(sums, A, R0s, R0d, Rd, constraint, weight=1.0, dr=None):
    """The epilogue's algebra in float64: loss = weight sum / (count n_ch); d / d R_s = sums[14:23], d / d R_d =
    sums[5:14], h = R_d sums[2:5] to d / d t_s and -h to d / d t_d, the rotation blocks through R = R0 Exp(dr).  Returns
    (loss, (d dr_s, d dt_s, d dr_d, d dt_d)) and the same four built from A with every matrix in absolute value.
    Rd: the destination's rotation the sums were taken at; dr: (dr_s, dr_d), zeros when left out."""
    sc = weight / (max(float(sums[1]), 1.0) * N_CH[constraint])
    Rd = torch.as_tensor(Rd, dtype=F64).reshape(3, 3)
    dr = (torch.zeros(3, dtype=F64),) * 2 if dr is None else dr
    out, bar = [], []
    for R0, blk, sign, w in ((R0s, slice(14, 23), 1.0, dr[0]), (R0d, slice(5, 14), -1.0, dr[1])):
        R0 = torch.as_tensor(R0, dtype=F64).reshape(3, 3)
        J = _exp_jacobian64(w)
        out += [torch.einsum("ijk,ij->k", J, R0.T @ sums[blk].view(3, 3)) * sc, sign * (Rd @ sums[2:5]) * sc]
        bar += [torch.einsum("ijk,ij->k", J.abs(), R0.T.abs() @ A[blk].view(3, 3)) * sc, (Rd.abs() @ A[2:5]) * sc]
    return float(sums[0]) * sc, out, bar


def mips_literal64(p, normals, feats_dst, bound, R0, t0, ws, bs, constraint, weight=1.0, mask=None, dr=None, dt=None,
                   stock=False, dtype=F64):
    """(loss, (d dr_s, d dt_s, d dr_d, d dt_d), rows kept) -- module docstring.  p (n,3) rows in the source frame, normals (n,3);
    R0 = (R0_s, R0_d) (3,3), t0 = (t0_s, t0_d) (3,); dr / dt: the corrections the derivative is taken at (pairs of (3,),
    zeros when left out).  mask (n,) bool: the rows kept, for a caller that holds the in-bound set (the kernel's); None:
    the float64 bound test at these poses.  stock: the destination's SDF through R.sdf_stock (an atlas submap) instead
    of R.sdf_gather.  dtype F32: the same operations in fp32 -- the op-by-op route's arithmetic, whose difference p -
    match_src cancels all of |p| -- for measuring that route's own rounding noise; the rows kept stay the float64 ones."""
    from miso_amd import so3
    assert constraint in CONSTRAINTS
    z = lambda v: (torch.zeros(3, dtype=dtype) if v is None else torch.as_tensor(v).to(dtype).reshape(3).clone()).requires_grad_(True)
    dr_s, dr_d = (z(None), z(None)) if dr is None else (z(dr[0]), z(dr[1]))
    dt_s, dt_d = (z(None), z(None)) if dt is None else (z(dt[0]), z(dt[1]))
    f64 = lambda v: torch.as_tensor(v).to(dtype)
    Rs = f64(R0[0]).reshape(3, 3) @ so3.so3_exp_map(dr_s.view(1, 3))[0]
    Rd = f64(R0[1]).reshape(3, 3) @ so3.so3_exp_map(dr_d.view(1, 3))[0]
    ts, td = f64(t0[0]).reshape(3) + dt_s, f64(t0[1]).reshape(3) + dt_d
    b = f64(bound)
    pts, nv = f64(p), f64(normals)
    if mask is None:
        with torch.no_grad():
            q0 = ((p.double() @ Rs.double().T + ts.double()) - td.double()) @ Rd.double()
            mask = ((q0 >= b.double()[:, 0]) & (q0 <= b.double()[:, 1])).all(1)
    pts, nv = pts[mask], nv[mask]
    q = ((pts @ Rs.T + ts) - td) @ Rd                                   # transform_points_to, transfrom_points_from
    sdf = R.sdf_stock if stock else R.sdf_gather
    s = sdf([f64(f) for f in feats_dst], b, q, [f64(w) for w in ws], [None if v is None else f64(v) for v in bs])
    (g,) = torch.autograd.grad(s.sum(), q, retain_graph=True)
    match_dst = q - s * g.detach()
    match_src = ((match_dst @ Rd.T + td) - ts) @ Rs
    cons = ((pts - match_src) * nv).sum(1) if constraint == "point_to_plane" else pts - match_src
    loss = weight * torch.mean(cons ** 2)
    grads = torch.autograd.grad(loss, [dr_s, dt_s, dr_d, dt_d])
    return float(loss.detach()), [v.detach() for v in grads], int(mask.sum())
