"""Decoder weight gradients in HIP (miso_amd/csrc/decoder_wgrad.hip, ops.sdf_wgrad_raw) and the trainable decoder on the
fused route (ops._SdfFusedTrainable, GridNet.forward).

Truth is FLOAT64: the oracle's stock encode + the decoder as matrix products, CPU, double autograd.  The yardstick for an
fp32 result is what a trainable decoder ran before the kernel existed, on the same inputs and the same device: ops.encode
+ torch.nn.functional.linear (ops._mlp_torch) under torch autograd.  The bar is the one of tests/test_split_precision.py
(lines 113-114): for every dW_l and db_l

    max |hip - f64|  <= 2 max |torch_fp32 - f64|  + 1e-7 scale,     mean |hip - f64| <= 2 mean |torch_fp32 - f64| + 2e-9 scale

with scale = max |f64|.  ReLU ties (a pre-activation within TIE = 1e-6 of zero in float64) may be gated differently by any
two fp32 evaluations; such points carry a zero cotangent, and where the test says so their share is capped first.
Arithmetic compared: grid_opt/models/modules.py:11-32 (MLPNet), training/train_decoder.py:73-179 (what trains it).
"""
import os
import subprocess
import sys

import pytest
import torch

import test_split_precision as S
from oracle import ref_torch as R

pytestmark = pytest.mark.gpu
DEV = S.DEV
TIE = S.TIE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = [[-1.0, 1.0]] * 3


def _inputs(monkeypatch, n, levels, C, H, bound, dyadic, seed, bias=True):
    """test_split_precision._inputs at n points (it reads its module's N)"""
    monkeypatch.setattr(S, "N", n)
    x, feats, b, ws, bs, g = S._inputs(levels, C, H, bound, dyadic, seed)
    return x, feats, b, ws, (bs if bias else [None] * len(ws)), g


def _chain(rows, ws, bs):
    """-> (sdf, pre-activations) of the decoder as matrix products"""
    pre, h = [], rows
    for i, (w, b) in enumerate(zip(ws, bs)):
        h = h @ w.T if b is None else h @ w.T + b
        if i + 1 < len(ws):
            pre.append(h)
            h = torch.relu(h)
    return h, pre


class Oracle64:
    """float64 forward kept as a graph: the tie census, then gradients for a cotangent"""

    def __init__(self, x, feats, b, ws, bs, ignore=None):
        self.x = x.double().requires_grad_(True)
        self.f = [f.double().requires_grad_(True) for f in feats]
        self.w = [w.double().requires_grad_(True) for w in ws]
        self.b = [None if v is None else v.double().requires_grad_(True) for v in bs]
        rows = R.encode_stock(self.f, b.double(), self.x, ignore)
        self.sdf, pre = _chain(rows, self.w, self.b)
        self.near = torch.stack([p.detach().abs().min(dim=1).values for p in pre]).min(dim=0).values < TIE

    def grads(self, g):
        """d (sum g sdf) / d (weights, biases): -> ([dW_l], [db_l or None])"""
        params = self.w + [v for v in self.b if v is not None]
        got = list(torch.autograd.grad(self.sdf, params, g.double(), retain_graph=True))
        gw = [got.pop(0) for _ in self.w]
        return gw, [None if v is None else got.pop(0) for v in self.b]


def _on_device(x, feats, b, ws, bs, ignore=None):
    from miso_amd import ops
    meta = ops.GridMeta.from_bound(b, ignore)
    fd = [f.to(DEV).contiguous(memory_format=torch.channels_last_3d) for f in feats]
    wd = [w.to(DEV) for w in ws]
    bd = [None if v is None else v.to(DEV) for v in bs]
    return meta, fd, wd, bd, x.to(DEV)


def _torch_fp32(meta, fd, wd, bd, xd, g):
    """the yardstick: encode + F.linear under torch autograd, on the device"""
    from miso_amd import ops
    ws = [w.clone().requires_grad_(True) for w in wd]
    bs = [None if v is None else v.clone().requires_grad_(True) for v in bd]
    out = ops._mlp_torch(ops.encode(xd, fd, meta), ws, bs)
    got = list(torch.autograd.grad(out, ws + [v for v in bs if v is not None], g.to(DEV)))
    gw = [got.pop(0) for _ in ws]
    return gw, [None if v is None else got.pop(0) for v in bs]


def _hip(meta, fd, wd, bd, xd, g, exact=False, binned=None):
    """forward (sign bits) + the weight-gradient kernel.  binned: None, 'caller' (gsdf in caller order) or 'sorted'"""
    from miso_amd import ops
    pack = ops.DecoderPack(wd, bd)
    gd = g.to(DEV)
    sb = None if binned is None else ops.SortedBatch(xd.shape[0], xd.device).sort(xd, meta)
    with ops.exact_fp32(exact):
        _, mask = ops.sdf_fwd_raw(xd, fd, meta, pack, want_mask=True, sorted_batch=sb)
    if binned == "sorted":
        gd = gd.index_select(0, sb.perm.long())
    out = ops.sdf_wgrad_raw(xd, fd, meta, pack, gd, mask, sorted_batch=sb, gsdf_sorted=binned == "sorted")
    torch.cuda.synchronize()
    return out


def _within_bar(tag, hip, t32, ref):
    """the bar of test_split_precision.py:113-114; every figure is printed before it is asserted"""
    names = [f"dW{l}" for l in range(len(ref[0]))] + [f"db{l}" for l in range(len(ref[1]))]
    for what, h, t, r in zip(names, hip[0] + hip[1], t32[0] + t32[1], ref[0] + ref[1]):
        assert (h is None) == (r is None), f"{tag} {what}"
        if r is None:
            continue
        h, t = h.detach().cpu().double(), t.detach().cpu().double()
        assert h.shape == r.shape and bool(torch.isfinite(h).all()), f"{tag} {what}"
        (hmax, hmean), (tmax, tmean) = S._err(h, r), S._err(t, r)
        scale = r.abs().max().item()
        line = (f"{tag} {what}: hip max {hmax:.3e} mean {hmean:.3e} | torch fp32 max {tmax:.3e} mean {tmean:.3e} "
                f"| scale {scale:.3e}")
        print(line)
        assert hmax <= 2.0 * tmax + 1e-7 * scale, line
        assert hmean <= 2.0 * tmean + 2e-9 * scale, line


# (name, level sizes (Z,Y,X), C, H, bound, dyadic): cfg1_dyadic, cfg2, cfg3 of test_split_precision.py and (8, 3, 32)
BY_NAME = {s[0]: s for s in S.SHAPES}
SHAPES = [BY_NAME["cfg1_dyadic"], BY_NAME["cfg2"], BY_NAME["cfg3"],
          ("c8_l3_h32", [(16, 16, 16), (32, 32, 32), (64, 64, 64)], 8, 32, UNIT, False)]
N_BIG = 70001      # not a multiple of 64; 1094 chunks over 256 partial blocks: the accumulators carry over chunks


def _case(monkeypatch, shape, n, seed, cap=True, bias=True):
    name, levels, C, H, bound, dyadic = shape
    x, feats, b, ws, bs, g = _inputs(monkeypatch, n, levels, C, H, bound, dyadic, seed, bias)
    o = Oracle64(x, feats, b, ws, bs)
    if cap:
        assert int(o.near.sum()) < 0.01 * n      # the precondition, before the cotangent is zeroed
    g = g.clone()
    g[o.near] = 0.0
    return o, g, _on_device(x, feats, b, ws, bs)


@pytest.mark.parametrize("exact", [False, True], ids=["split_fwd", "exact_fwd"])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_weight_gradients_against_float64(monkeypatch, shape, exact):
    """1. every dW_l and db_l within the bar, the forward (whose sign bits gate the kernel) in either arithmetic"""
    o, g, dev = _case(monkeypatch, shape, N_BIG, seed=len(shape[0]) * 7 + shape[2])
    _within_bar(f"{shape[0]} exact={exact}", _hip(*dev, g, exact=exact), _torch_fp32(*dev, g), o.grads(g))


SMALL = [("c4_l1_h32", [(12, 10, 14)], 4, 32, UNIT, False),                                  # F = 4, one row tile
         ("c8_l4_h64", [(6, 6, 6), (10, 10, 10), (12, 14, 16), (20, 20, 20)], 8, 64, UNIT, False)]   # F = 32: no padding columns


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("shape", SMALL, ids=[s[0] for s in SMALL])
def test_smallest_shapes(monkeypatch, shape, n, bias):
    """2. one wavefront and less, a full chunk, one point more, four chunks (one per wave of a workgroup: the sum
    over waves); with and without biases.  More than one workgroup: the n = 20 000 and 70 001 tests below"""
    o, g, dev = _case(monkeypatch, shape, n, seed=n + shape[3], cap=False, bias=bias)
    hip = _hip(*dev, g)
    assert all((v is None) == (not bias) for v in hip[1])
    _within_bar(f"{shape[0]} n={n} bias={bias}", hip, _torch_fp32(*dev, g), o.grads(g))


@pytest.mark.parametrize("shape", SMALL, ids=[s[0] for s in SMALL])
def test_points_outside_ignored_level_and_sparse_cotangent(monkeypatch, shape):
    """2. (the three single cases) zeros padding, ignore_mask, a cotangent that is zero on half the rows"""
    name, levels, C, H, bound, dyadic = shape
    n = 200
    x, feats, b, ws, bs, g = _inputs(monkeypatch, n, levels, C, H, bound, dyadic, seed=11)
    # every point outside the bound: the feature rows are zero, so dW_0 is, and nothing is NaN
    x_out = x + 4.0
    o = Oracle64(x_out, feats, b, ws, bs)
    g0 = g.clone()
    g0[o.near] = 0.0
    dev = _on_device(x_out, feats, b, ws, bs)
    hip = _hip(*dev, g0)
    assert torch.count_nonzero(hip[0][0]).item() == 0
    _within_bar(f"{name} outside", hip, _torch_fp32(*dev, g0), o.grads(g0))
    # one level ignored: its columns of dW_0 are exactly zero
    ignore = [l == len(levels) - 1 for l in range(len(levels))]
    o = Oracle64(x, feats, b, ws, bs, ignore)
    g1 = g.clone()
    g1[o.near] = 0.0
    dev = _on_device(x, feats, b, ws, bs, ignore)
    hip = _hip(*dev, g1)
    assert torch.count_nonzero(hip[0][0][:, C * (len(levels) - 1):]).item() == 0
    if len(levels) > 1:
        assert torch.count_nonzero(hip[0][0][:, :C]).item() > 0
    _within_bar(f"{name} ignore", hip, _torch_fp32(*dev, g1), o.grads(g1))
    # a cotangent that is zero on every other row
    o = Oracle64(x, feats, b, ws, bs)
    g2 = g.clone()
    g2[o.near] = 0.0
    g2[::2] = 0.0
    dev = _on_device(x, feats, b, ws, bs)
    _within_bar(f"{name} half", _hip(*dev, g2), _torch_fp32(*dev, g2), o.grads(g2))


@pytest.mark.parametrize("n", [20000, N_BIG])
def test_binned_order_equals_caller_order(monkeypatch, n):
    """3. a binned forward's sign bits + the kernel on the binned batch, d sdf in the caller's order and in the binned one:
    the three differ in the order of fp32 sums only, so each is held against float64"""
    o, g, dev = _case(monkeypatch, BY_NAME["cfg2"], n, seed=n % 97)
    ref, t32 = o.grads(g), _torch_fp32(*dev, g)
    for binned in (None, "caller", "sorted"):
        _within_bar(f"cfg2 n={n} binned={binned}", _hip(*dev, g, binned=binned), t32, ref)


@pytest.mark.parametrize("binned", [None, "caller"], ids=["unbinned", "binned"])
def test_two_calls_return_the_same_bits(monkeypatch, binned):
    """4. no atomics, fixed order of the partial sums"""
    from miso_amd import ops
    o, g, (meta, fd, wd, bd, xd) = _case(monkeypatch, BY_NAME["cfg2"], N_BIG, seed=3)
    pack, gd = ops.DecoderPack(wd, bd), g.to(DEV)
    sb = None if binned is None else ops.SortedBatch(N_BIG, xd.device).sort(xd, meta)      # ONE binning: the calls are identical
    _, mask = ops.sdf_fwd_raw(xd, fd, meta, pack, want_mask=True, sorted_batch=sb)
    a, b = (ops.sdf_wgrad_raw(xd, fd, meta, pack, gd, mask, sorted_batch=sb) for _ in range(2))
    torch.cuda.synchronize()
    for u, v in zip(a[0] + a[1], b[0] + b[1]):
        assert torch.equal(u, v)
    assert all(bool(u.abs().max() > 0) for u in a[0])


# ---- the model -------------------------------------------------------------------------------------------------------
def _gridnet(fix, seed=0, C=8, L=3, H=64):
    from miso_amd.grid_opt.models.grid_net import GridNet
    cfg = {"name": "grid_net", "spatial_dim": 3,
           "decoder": {"type": "mlp", "hidden_dim": H, "hidden_layers": 1, "out_dim": 1, "pos_invariant": True,
                       "fix": fix, "pretrained_model": None},
           "grid": {"type": "regular", "feature_dim": C, "init_stddev": 3e-2, "bound": UNIT, "base_cell_size": 0.25,
                    "per_level_scale": 2, "n_levels": L},
           "pose": {"optimize": False, "num_poses": 1}}
    torch.manual_seed(seed)
    net = GridNet(cfg, device=DEV).to(DEV)
    net.unlock_feature()
    return net


def _params(net):
    lin = net.decoder.linears()
    return [g.feature for g in net.features], [m.weight for m in lin], [m.bias for m in lin]


def _points(n, seed):
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)) * 1.9 - 0.95


def _backward(net, x, route):
    """loss = mean |sdf| through net.forward on the fused (True) or the op-by-op (False) route -> (sdf, gradients)"""
    import miso_amd.grid_opt.models.grid_net as GN
    feats, ws, bs = _params(net)
    saved, GN._FUSED_WGRAD = GN._FUSED_WGRAD, route
    try:
        xd = x.to(DEV).requires_grad_(True)
        sdf = net(xd)
        got = list(torch.autograd.grad(sdf.abs().mean(), [xd] + feats + ws + bs))
    finally:
        GN._FUSED_WGRAD = saved
    torch.cuda.synchronize()
    return sdf.detach(), got


def test_autograd_end_to_end(monkeypatch):
    """5. GridNet with a trainable decoder: x, every level and every decoder parameter within the bar; the switch is
    connected; a frozen decoder is ops._SdfFused bit for bit"""
    from miso_amd import ops
    n = 5000
    net = _gridnet(fix=False)
    feats, ws, bs = _params(net)
    assert all(p.requires_grad for p in ws + bs)
    x = _points(n, 1)
    calls = []
    real = ops.sdf_wgrad_raw
    monkeypatch.setattr(ops, "sdf_wgrad_raw", lambda *a, **k: calls.append(1) or real(*a, **k))
    sdf_f, got_f = _backward(net, x, True)
    assert calls, "a trainable decoder did not take the fused route"
    sdf_t, got_t = _backward(net, x, False)
    assert len(calls) == 1, "_FUSED_WGRAD = False did not restore the torch route"
    assert not torch.equal(sdf_f, sdf_t), "both routes returned the same bits: is the switch connected?"
    assert (sdf_f - sdf_t).abs().max().item() <= 1e-5
    o = Oracle64(x, [f.detach().cpu() for f in feats], net.bound.detach().cpu(), [w.detach().cpu() for w in ws],
                 [v.detach().cpu() for v in bs])
    ref = list(torch.autograd.grad(o.sdf.abs().mean(), [o.x] + o.f + o.w + o.b))
    k = 1 + len(feats)
    _within_bar("gridnet x, levels", (got_f[:k], []), (got_t[:k], []), (ref[:k], []))
    _within_bar("gridnet decoder", (got_f[k:k + 3], got_f[k + 3:]), (got_t[k:k + 3], got_t[k + 3:]), (ref[k:k + 3], ref[k + 3:]))

    # frozen: GridNet.forward is ops._SdfFused, bit for bit.  Grid gradients are sums over points whose order is not
    # reproducible between two calls of ANY one code path (float atomics below the binning size, the binning's own order
    # above it), so the points are placed where the question has an answer: no two of them share a vertex at any level,
    # every gradient element is then one product added to zero.  Checked, not assumed.
    frozen = _gridnet(fix=True)
    feats, ws, bs = _params(frozen)
    assert not any(p.requires_grad for p in ws + bs)
    gen = torch.Generator().manual_seed(2)
    xs = torch.cartesian_prod(*[torch.tensor([-0.7, 0.0, 0.7])] * 3) + (torch.rand(27, 3, generator=gen) - 0.5) * 0.06
    for f in feats:
        size = torch.tensor([f.shape[4], f.shape[3], f.shape[2]], dtype=torch.float64)      # X, Y, Z
        i0 = torch.floor((xs.double() + 1) / 2 * size - 0.5)
        assert bool(((i0[:, None, :] - i0[None, :, :]).abs().max(dim=-1).values + 2 * torch.eye(27) >= 2).all())
    xb = xs.to(DEV)
    meta = frozen.features[0].grid_meta(frozen.ignore_level_)
    outs = []
    for call in (lambda q: frozen(q), lambda q: ops._SdfFused.apply(q, meta, frozen.decoder.decoder_pack(), *feats)):
        xq = xb.clone().requires_grad_(True)
        sdf = call(xq)
        outs.append([sdf.detach()] + list(torch.autograd.grad(sdf.abs().mean(), [xq] + feats)))
    assert len(calls) == 1
    for a, c in zip(*outs):
        assert bool(a.abs().max() > 0) and torch.equal(a, c)


def test_repack_after_an_in_place_step():
    """6. optimizer.step() on the decoder is seen by the next forward"""
    from miso_amd import ops
    net = _gridnet(fix=False)
    feats, ws, bs = _params(net)
    x = _points(3000, 4).to(DEV)
    opt = torch.optim.Adam(net.decoder.parameters(), lr=1e-2)
    before = net(x)
    before.abs().mean().backward()
    assert all(p.grad is not None and bool(p.grad.abs().max() > 0) for p in ws + bs)
    before = before.detach().clone()
    opt.step()
    after = net(x).detach()
    fresh = ops.DecoderPack([w.detach().clone() for w in ws], [v.detach().clone() for v in bs])
    meta = net.features[0].grid_meta(net.ignore_level_)
    want, _ = ops.sdf_fwd_raw(x, [f.detach() for f in feats], meta, fresh, want_mask=False)
    assert torch.equal(after, want)
    assert not torch.equal(after, before)


def test_shared_decoder_gradients_add_up():
    """7. two GridNets share one MLPNet (what pretraining does: a decoder over several scenes).  One backward over the sum
    of both losses = the sum of two separate backward passes, to the order of two fp32 additions (1e-6 scale).  One
    batch is of binning size: the kernel then runs on the binned batch with d sdf in the caller's order."""
    a, b = _gridnet(fix=False, seed=1), _gridnet(fix=False, seed=2)
    b.decoder = a.decoder
    xa, xb = _points(N_BIG, 5).to(DEV), _points(3000, 6).to(DEV)
    params = list(a.decoder.parameters())
    la, lb = a(xa).abs().mean(), b(xb).abs().mean()
    ga, gb = torch.autograd.grad(la, params), torch.autograd.grad(lb, params)
    both = torch.autograd.grad(a(xa).abs().mean() + b(xb).abs().mean(), params)
    for u, v, w in zip(ga, gb, both):
        want = u + v
        assert bool(u.abs().max() > 0) and bool(v.abs().max() > 0)
        assert (w - want).abs().max().item() <= 1e-6 * want.abs().max().item()


def test_create_graph_with_a_trainable_decoder(monkeypatch):
    """8. the eikonal step of tools/eikonal_bench.py (n = 3000) with weights that take a gradient: the second backward goes
    through the graph rebuilt in torch; grids and weights against float64 double autograd.  ReLU-tie points carry no
    weight in the loss (as in test_split_precision.py::test_fused_double_backward_equals_the_torch_linear_chain)."""
    from miso_amd import ops
    name, levels, C, H, bound, dyadic = BY_NAME["cfg2"]
    n = 3000
    x, feats, b, ws, bs, _ = _inputs(monkeypatch, n, levels, C, H, bound, dyadic, seed=8)
    x = x * 0.95
    o = Oracle64(x, feats, b, ws, bs)
    keep = (~o.near).double()
    sdf64 = R.sdf_gather(o.f, b.double(), o.x, o.w, o.b)
    g64, = torch.autograd.grad(sdf64.sum(), o.x, create_graph=True)
    loss64 = (keep * (g64.norm(dim=1) - 1) ** 2).mean() + (keep * sdf64.abs().view(-1)).mean()
    ref = list(torch.autograd.grad(loss64, o.f + o.w + o.b))

    meta, fd, wd, bd, xd = _on_device(x, feats, b, ws, bs)
    keep_d = keep.float().to(DEV)
    leaves = [t.clone().requires_grad_(True) for t in fd + wd + bd]
    L = len(fd)

    def run(fused):
        f_, w_, b_ = leaves[:L], leaves[L:L + 3], leaves[L + 3:]
        xq = xd.clone().requires_grad_(True)
        if fused:
            pack = ops.DecoderPack(w_, b_)
            assert pack.trainable()
            sdf = ops.sdf_fused(xq, f_, meta, pack)
        else:
            sdf = ops._mlp_torch(ops.encode(xq, f_, meta), w_, b_)
        with ops.coordinate_gradient_only():
            g, = torch.autograd.grad(sdf.sum(), xq, create_graph=True)
        loss = (keep_d * (g.norm(dim=1) - 1) ** 2).mean() + (keep_d * sdf.abs().view(-1)).mean()
        return list(torch.autograd.grad(loss, leaves))

    hip, t32 = run(True), run(False)
    _within_bar("eikonal levels", (hip[:L], []), (t32[:L], []), (ref[:L], []))
    _within_bar("eikonal decoder", (hip[L:L + 3], hip[L + 3:]), (t32[L:L + 3], t32[L + 3:]), (ref[L:L + 3], ref[L + 3:]))


def test_pretraining_tool_smoke(tmp_path):
    """9. tools/pretrain_decoder_synthetic.py, 2 scenes, 30 steps, in a child process: a loadable decoder.pt, and the
    loss went down (a direction, not a threshold)"""
    out = tmp_path / "decoder.pt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pretrain_decoder_synthetic.py"), "--scenes", "2",
                        "--steps", "30", "--points", "8192", "--out", str(out)], capture_output=True, text=True,
                       timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(l.split("loss")[1].split()[0]) for l in r.stdout.splitlines() if l.startswith("step")]
    assert len(losses) >= 2 and losses[-1] < losses[0], r.stdout[-2000:]
    sd = torch.load(out, map_location="cpu")
    assert {"network.0.weight", "network.2.weight", "network.4.weight"} <= set(sd)
    assert "frozen fused path: ok" in r.stdout
