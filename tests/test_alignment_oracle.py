"""The fp64 alignment oracle itself (oracle.ref_torch.pair_latent_sums64 and its comparison helper), without a GPU.

* Two oracles: pair_latent_sums64 (its own trilinear value and derivative, its own chain rule) against fp64 autograd
  through pairwise_latent_loss (encode_stock: F.grid_sample and ATen's backward, the reference's op order).  They share
  no interpolation code, and agree to 1e-9 of the absolute-value yardstick A on vertices kept 1e-3 index units from
  every cell plane and 1e-4 m from every face.
* Sensitivity: the bar the GPU tests hold the kernels to (count exact, |kernel - fp64| <= 1e-5 A + 1e-12) must reject a
  dropped vertex, a wrong level offset, a flipped gradient sign on 1 % of the vertices and a count off by one, and must
  accept the oracle's own fp32 evaluation at the same coordinates.
"""
import numpy as np
import pytest
import torch

import golden_cases as gc
from oracle import ref_torch as R

F32, F64 = torch.float32, torch.float64

BOUND = [[-4.0, 4.0], [-2.0, 3.0], [-3.0, 3.5]]
SHAPES = [(1, 4, 7, 5, 8), (1, 4, 13, 10, 16)]          # (1,C,Z,Y,X): two levels, odd and non-cubic


def _pose(seed, dt=(0.3, -0.2, 0.1)):
    rs = np.random.RandomState(seed)
    Rs = torch.tensor(gc.rodrigues(rs.uniform(-0.3, 0.3, 3)), dtype=F32)
    Rd = torch.tensor(gc.rodrigues(rs.uniform(-0.3, 0.3, 3)), dtype=F32)
    ts = torch.tensor(rs.uniform(-0.5, 0.5, 3), dtype=F32)
    td = ts + torch.tensor(dt, dtype=F32)
    return torch.cat([Rs.flatten(), ts, Rd.flatten(), td])


def _safe_vertices(n, pose64, g):
    """Source vertices whose exact map lands 1e-4 m or more from every face of BOUND (inside and outside) and 1e-3
    index units or more from every cell plane of every level."""
    Rs, ts, Rd, td = pose64[:9].view(3, 3), pose64[9:12], pose64[12:21].view(3, 3), pose64[21:24]
    b = torch.tensor(BOUND, dtype=F64)
    out = torch.empty(0, 3, dtype=F64)
    while out.shape[0] < n:
        q = (torch.rand(4 * n, 3, generator=g, dtype=F64) * 1.2 - 0.1) * (b[:, 1] - b[:, 0]) + b[:, 0]
        p = ((q @ Rd.T + td - ts) @ Rs).float().double()          # Rs^T (Rd q + td - ts), rounded to fp32
        q = (p @ Rs.T + (ts - td)) @ Rd
        ok = ((q - b[:, 0]).abs() > 1e-4).all(1) & ((q - b[:, 1]).abs() > 1e-4).all(1)
        xn = R.normalize_coordinates(q, b)
        for s in SHAPES:
            ok &= R.fd_safe(xn, (s[4], s[3], s[2]), False, margin=1e-3)
        out = torch.cat([out, p[ok]])
    return out[:n]


@pytest.mark.parametrize("loss_type", ["L2", "L1"])
@pytest.mark.parametrize("nlev", [1, 2])
def test_pair_sums_agree_with_autograd_through_the_reference(loss_type, nlev):
    g = torch.Generator().manual_seed(7 + nlev)
    pose = _pose(3 + nlev).double()
    fsrc_grids = [torch.randn(s, generator=g, dtype=F64) * 0.1 for s in SHAPES[:nlev]]
    fdst = [torch.randn(s, generator=g, dtype=F64) * 0.1 for s in SHAPES[:nlev]]
    b = torch.tensor(BOUND, dtype=F64)
    p = _safe_vertices(3000, pose, g)
    fs = R.encode_stock(fsrc_grids, b, p)
    sums, A = R.pair_latent_sums64(p, fs, fdst, BOUND, pose, loss_type, exact=True)
    assert 200 < sums[1] < 3000                                      # some vertices in, some out
    ps = [pose[:9].view(3, 3).clone(), pose[9:12].view(3, 1).clone(), pose[12:21].view(3, 3).clone(),
          pose[21:24].view(3, 1).clone()]
    ps = [t.requires_grad_(True) for t in ps]
    loss = R.pairwise_latent_loss(fsrc_grids, b, fdst, b, p, *ps, level=nlev - 1, fdim=4, align_weight=1.0,
                                  align_loss=loss_type)
    grads = torch.autograd.grad(loss, ps)
    n_ch = 4 * nlev
    want = R.pair_pose_grads64(sums, pose[12:21], loss_type, n_ch)
    denom = max(float(sums[1]), 1.0) * (n_ch if loss_type == "L2" else 1)
    bars = (A[0] / denom, A[14:23].view(3, 3) / denom, None, A[5:14].view(3, 3) / denom, None)
    # the translation gradients: h = Rd G, its yardstick |Rd| A_G
    hA = (pose[12:21].view(3, 3).abs() @ A[2:5]).view(3, 1) / denom
    bars = (bars[0], bars[1], hA, bars[3], hA)
    for name, got, ref, bar in zip(("loss", "R_s", "t_s", "R_d", "t_d"), (loss,) + grads, want, bars):
        err = (torch.as_tensor(got) - ref).abs()
        assert (err <= 1e-9 * bar + 1e-15).all(), (name, err, bar)


def _sensitivity_case(loss_type="L2"):
    g = torch.Generator().manual_seed(11)
    pose = _pose(5)
    fdst = [torch.randn(s, generator=g) * 0.1 for s in SHAPES]
    # 2 049 source vertices, every one of them in bound
    b = torch.tensor(BOUND, dtype=F64)
    p = _safe_vertices(6000, pose.double(), g).float()
    _, _, m = R.src_to_dst32(p, pose[:9], pose[9:12], pose[12:21], pose[21:24], BOUND)
    p = p[m][:2049]
    assert p.shape[0] == 2049
    fsrc = torch.randn(2049, 8, generator=g) * 0.1
    return p, fsrc, fdst, pose


@pytest.mark.parametrize("loss_type", ["L2", "L1"])
def test_the_pair_bar_sees_what_it_must(loss_type):
    p, fsrc, fdst, pose = _sensitivity_case(loss_type)
    sums, A = R.pair_latent_sums64(p, fsrc, fdst, BOUND, pose, loss_type)
    assert sums[1] == 2049
    sums_only = lambda ex: ex[[0] + list(range(2, 23))]
    # the oracle's own fp32 evaluation at the same coordinates passes
    s32, _ = R.pair_latent_sums64(p, fsrc, fdst, BOUND, pose, loss_type, dtype=F32)
    ex = R.pair_sums_excess(s32, sums, A)
    assert (ex <= 0).all(), ex
    # one vertex dropped (the count patched back: the sums alone must see it)
    drop, _ = R.pair_latent_sums64(torch.cat([p[:1000], p[1001:]]), torch.cat([fsrc[:1000], fsrc[1001:]]), fdst,
                                   BOUND, pose, loss_type)
    drop[1] = sums[1]
    assert (sums_only(R.pair_sums_excess(drop, sums, A)) > 0).any()
    # one vertex read with the wrong level offset (its level-1 channels taken from level 0's)
    bad = fsrc.clone()
    bad[700, 4:8] = fsrc[700, 0:4]
    off, _ = R.pair_latent_sums64(p, bad, fdst, BOUND, pose, loss_type)
    assert (sums_only(R.pair_sums_excess(off, sums, A)) > 0).any()
    # the count off by one
    one = sums.clone()
    one[1] += 1
    assert R.pair_sums_excess(one, sums, A)[1] > 0
    # the sign of level 1's share of the gradient flipped on 1 % of the vertices (recomputed per vertex: L1's
    # derivative -r / |r| couples the levels through the norm)
    sign = torch.ones(2049, 2)
    sign[::100, 1] = -1.0
    flip, _ = R.pair_latent_sums64(p, fsrc, fdst, BOUND, pose, loss_type, level_sign=sign)
    assert torch.equal(flip[:2], sums[:2])
    assert (sums_only(R.pair_sums_excess(flip, sums, A)) > 0).any()


def test_src_to_dst32_is_exact_on_dyadic_geometry():
    """Signed-permutation rotations, dyadic translations and vertices: every step of the fp32 map is exact."""
    g = torch.Generator().manual_seed(2)
    p = torch.randint(-512, 512, (1000, 3), generator=g).float() / 64
    Rs = torch.tensor([[0., -1, 0], [0, 0, 1], [-1, 0, 0]])
    Rd = torch.tensor([[0., 0, 1], [1, 0, 0], [0, 1, 0]])
    ts, td = torch.tensor([0.5, -1.25, 2.0]), torch.tensor([-0.75, 0.125, 1.5])
    d, q, m = R.src_to_dst32(p, Rs, ts, Rd, td, BOUND)
    q64 = (p.double() @ Rs.double().T + (ts - td).double()) @ Rd.double()
    assert torch.equal(q.double(), q64)
    b = torch.tensor(BOUND, dtype=F64)
    assert torch.equal(m, ((q64 >= b[:, 0]) & (q64 <= b[:, 1])).all(1))
