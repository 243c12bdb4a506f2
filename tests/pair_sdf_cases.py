"""Inputs and the float64 oracle of the SDF pair stage (csrc/pair_sdf.hip; ops.AlignPlan(residual="sdf")), shared by
test_pair_sdf_host.py (no GPU: the oracle and its bar) and test_pair_sdf.py (the kernel against it).

pair_sdf_sums64 restates the 24 sums of miso_pair_latent for the SDF residual: the in-bound set and q are
R.src_to_dst32's (the kernel's own fp32 map, operation by operation), s = R.sdf_gather(dst levels, q) with the decoder
in ``dtype``, grad_q s by autograd, r = ref - s, the term and its derivative per loss type, then the sums.  Beside them
it returns the absolute-value yardstick A, as R.pair_latent_sums64 does: the same sums over |term| and |g|
(componentwise), with |d| = |Rs||p| + |ts - td| and |Rd||g| in the two 3x3 blocks.  (R.pair_latent_sums64 bounds |g|
from the corner values; here |g| itself is summed, which is never larger: the bar is no wider.)

The row lists are built like test_alignment_oracle._safe_vertices -- the exact map of every row lies 1e-4 m or more from
every face of the bound, inside or outside, and 1e-3 index units or more from every cell plane of every level, so the
count is a fair exact condition -- and, in bound, every hidden pre-activation of the decoder is 1e-4 or more away from
zero: d s / d q jumps where a ReLU switches, and a row that sits on such a switch to within rounding has no gradient
for an fp32 evaluation to agree with."""
import functools
import math

import numpy as np
import torch

import golden_cases as gc
from oracle import ref_torch as R

F32, F64 = torch.float32, torch.float64

BOUND = [[-4.0, 4.0], [-2.0, 3.0], [-3.0, 3.5]]
# the fused shapes (C, L, H) = (4, 2, 64) and (8, 1, 64): levels (1,C,Z,Y,X), odd and non-cubic
GRIDS = {"c4l2": [(1, 4, 7, 5, 8), (1, 4, 13, 10, 16)], "c8l1": [(1, 8, 9, 6, 11)]}
HIDDEN = 64
GM_SCALE = 0.1
RELU_MARGIN = 1e-4


def pose(seed, dt=(0.3, -0.2, 0.1)):
    rs = np.random.RandomState(seed)
    Rs = torch.tensor(gc.rodrigues(rs.uniform(-0.3, 0.3, 3)), dtype=F32)
    Rd = torch.tensor(gc.rodrigues(rs.uniform(-0.3, 0.3, 3)), dtype=F32)
    ts = torch.tensor(rs.uniform(-0.5, 0.5, 3), dtype=F32)
    td = ts + torch.tensor(dt, dtype=F32)
    return torch.cat([Rs.flatten(), ts, Rd.flatten(), td])


def decoder(fdim, g):
    """MLPNet(fdim, 1, HIDDEN, hidden_layers=1): weights (out,in) and biases, fp32"""
    dims = [(HIDDEN, fdim), (HIDDEN, HIDDEN), (1, HIDDEN)]
    ws = [torch.randn(d, generator=g) / math.sqrt(d[1]) for d in dims]
    bs = [torch.randn(d[0], generator=g) * 0.1 for d in dims]
    return ws, bs


def _min_preactivation(feats64, b64, q64, ws, bs):
    h = R.encode_gather(feats64, b64, q64)
    lo = torch.full((q64.shape[0],), float("inf"), dtype=F64)
    for w, b in zip(ws[:-1], bs[:-1]):
        z = h @ w.double().T + b.double()
        lo = torch.minimum(lo, z.abs().min(1).values)
        h = torch.relu(z)
    return lo


def safe_rows(n, pose64, shapes, g, feats, ws, bs, span=1.15):
    """n source rows (fp32 values): see the module docstring.  span 1.15: the candidates fill a box 1.15 times the
    bound per axis, so about a third of them (1 - 1.15^-3) map outside."""
    Rs, ts, Rd, td = pose64[:9].view(3, 3), pose64[9:12], pose64[12:21].view(3, 3), pose64[21:24]
    b = torch.tensor(BOUND, dtype=F64)
    feats64 = [f.double() for f in feats]
    out = torch.empty(0, 3, dtype=F64)
    while out.shape[0] < n:
        q = (torch.rand(4 * n + 64, 3, generator=g, dtype=F64) * span - 0.5 * (span - 1.0)) * (b[:, 1] - b[:, 0]) + b[:, 0]
        p = ((q @ Rd.T + td - ts) @ Rs).float().double()          # Rs^T (Rd q + td - ts), rounded to fp32
        q = (p @ Rs.T + (ts - td)) @ Rd
        ok = ((q - b[:, 0]).abs() > 1e-4).all(1) & ((q - b[:, 1]).abs() > 1e-4).all(1)
        xn = R.normalize_coordinates(q, b)
        for s in shapes:
            ok &= R.fd_safe(xn, (s[4], s[3], s[2]), False, margin=1e-3)
        inside = ((q >= b[:, 0]) & (q <= b[:, 1])).all(1)
        ok &= ~inside | (_min_preactivation(feats64, b, q, ws, bs) > RELU_MARGIN)
        out = torch.cat([out, p[ok]])
    return out[:n].float()


@functools.lru_cache(maxsize=None)
def case(grid, n, seed=0):
    """One pair: destination levels, decoder, pose, n source rows and their reference column (fp32, CPU)."""
    shapes = GRIDS[grid]
    g = torch.Generator().manual_seed(100 + 7 * seed + len(shapes))
    feats = [torch.randn(s, generator=g) * 0.3 for s in shapes]
    ws, bs = decoder(sum(s[1] for s in shapes), g)
    ps = pose(5 + seed)
    p = safe_rows(n, ps.double(), shapes, g, feats, ws, bs) if n else torch.zeros(0, 3)
    ref = torch.randn(n, generator=g) * 0.2
    return dict(grid=grid, feats=feats, ws=ws, bs=bs, pose=ps, p=p, ref=ref)


def pair_sdf_sums64(p, ref, feats_dst, bound, pose, weights, biases, loss_type="L2", gm_scale=GM_SCALE, dtype=F64,
                    g_sign=None):
    """(sums (24,) fp64, A (24,) fp64) -- module docstring.  dtype fp32: what a careful fp32 implementation computes at
    the same mapped coordinates (decoder, gradient and terms in fp32, summed in fp32 over runs of 8 rows like a kernel
    lane, then in fp64).  g_sign: optional (N,) of +-1 multiplying g per row -- the sums of a kernel that got the sign of
    the gradient wrong on those rows (sensitivity tests)."""
    pose = torch.as_tensor(pose, dtype=F32).reshape(24)
    Rs, ts, Rd, td = pose[:9].view(3, 3), pose[9:12], pose[12:21].view(3, 3), pose[21:24]
    sums, A = torch.zeros(24, dtype=F64), torch.zeros(24, dtype=F64)
    if p.shape[0] == 0:
        return sums, A
    _, q, m = R.src_to_dst32(p, Rs, ts, Rd, td, bound)
    idx = torch.nonzero(m).flatten()
    sums[1] = float(idx.numel())
    if idx.numel() == 0:
        return sums, A
    pi = p[idx].to(F32)
    b = torch.as_tensor(bound, dtype=F32).to(dtype)
    qi = q[idx].to(dtype).requires_grad_(True)
    s = R.sdf_gather([f.to(dtype) for f in feats_dst], b, qi, [w.to(dtype) for w in weights],
                     [None if v is None else v.to(dtype) for v in biases])[:, 0]
    (ds,) = torch.autograd.grad(s.sum(), qi)
    s = s.detach()
    r = torch.as_tensor(ref, dtype=F32).reshape(-1)[idx].to(dtype) - s
    if loss_type == "L2":
        term, coef = r * r, -2 * r
    elif loss_type == "L1":
        term, coef = r.abs(), -torch.sign(r)
    elif loss_type == "GM":
        w = gm_scale / (gm_scale + r * r) ** 2
        term, coef = w * r * r, -2 * w * r
    else:
        raise ValueError(loss_type)
    gq = coef[:, None] * ds
    if g_sign is not None:
        gq = gq * g_sign[idx].to(dtype)[:, None]

    def total(x):
        x = x.reshape(x.shape[0], -1)
        if dtype == F64:
            return x.sum(0)
        pad = (-x.shape[0]) % 8
        x = torch.cat([x, x.new_zeros(pad, x.shape[1])]).view(-1, 8, x.shape[1])
        return x.sum(1).double().sum(0)

    Rs64, ts64, Rd64, td64, p64 = Rs.double(), ts.double(), Rd.double(), td.double(), pi.double()
    dvec = p64 @ Rs64.T + (ts64 - td64)
    dabs = p64.abs() @ Rs64.abs().T + (ts64 - td64).abs()
    sums[0], A[0] = total(term)[0], total(term.abs())[0]
    sums[2:5], A[2:5] = total(gq), total(gq.abs())
    if dtype == F64:
        sums[5:14] = (dvec[:, :, None] * gq[:, None, :]).sum(0).flatten()
        sums[14:23] = ((gq @ Rd64.T)[:, :, None] * p64[:, None, :]).sum(0).flatten()
    else:       # the kernel's decomposition: S = sum p (x) g in fp32, then Rs S + (ts - td) G and Rd S^T in fp64
        S = total(pi[:, :, None] * gq[:, None, :]).view(3, 3)
        sums[5:14] = (Rs64 @ S + (ts64 - td64)[:, None] * sums[2:5][None, :]).flatten()
        sums[14:23] = (Rd64 @ S.T).flatten()
    ga = gq.abs().double()
    A[5:14] = (dabs[:, :, None] * ga[:, None, :]).sum(0).flatten()
    A[14:23] = ((ga @ Rd64.abs().T)[:, :, None] * p64.abs()[:, None, :]).sum(0).flatten()
    return sums, A


REL = 1e-4      # the d/dx bar of test_hip_parity.py::test_sdf_fused_vs_golden, applied term by term


def excess(got, sums, A):
    """R.pair_sums_excess at the SDF stage's bar: count exact, the others |got - fp64| <= 1e-4 A + 1e-12."""
    return R.pair_sums_excess(got, sums, A, rel=REL)
