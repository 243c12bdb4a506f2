"""ops.hash_sdf_* on the GPU, by identity with routes the suite already holds to float64 and by bounds it already derives:

  forward    the bits (SDF and ReLU sign words) of ops.sdf_fwd_raw on the dense twins D[k, j, i, :] = T[row(i, j, k)] of the
             tables (tests/hash_cases.py) -- the regular fused route, checked in tests/test_split_precision.py
  backward   its d-feat rows are the bits of ops.sdf_bwd_rows_raw on the dense twin (the same decoder chain), grad_x the
             bits of ops.hash_encode_bwd_raw fed those rows, and every table gradient lies within m 2^-24 sum |terms| of
             the float64 sum of the kernel's fp32 terms (hash_cases.table_gradient64: the bound of tests/test_hash_encode.py)

Shapes: the two levels of hash_cases.DIMS behind 2^6 and 2^8 rows, (C, H) = (4, 32), (4, 64), (8, 64), batch sizes
around the wavefront and the workgroup, every point kind, both decoder arithmetics."""
import functools
import os

import numpy as np
import pytest
import torch

import hash_cases as hc
import sampler_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = ((4, 32), (4, 64), (8, 64))
ARITH = (pytest.param(False, id="split", marks=pytest.mark.skipif(
    bool(os.environ.get("MISO_EXACT_F32")), reason="MISO_EXACT_F32 forces the exact chains: the split half is the other half")),
    pytest.param(True, id="exact"))


def _meta(ignore=None, flags=0):
    from miso_amd import ops
    return ops.GridMeta.from_bound(sc.BOUNDS[hc.BOUND], ignore, flags)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _weights(C, H, trainable=False):
    """a seeded Linear stack 2C - H - H - 1 with the first layer scaled as in test_split_precision._inputs"""
    torch.manual_seed(100 + C + H)
    lin = [torch.nn.Linear(2 * C, H), torch.nn.Linear(H, H), torch.nn.Linear(H, 1)]
    ws = [l.weight.detach().clone() for l in lin]
    bs = [l.bias.detach().clone() for l in lin]
    ws[0] = ws[0] * 8.0
    return [w.to(DEV).requires_grad_(trainable) for w in ws], [b.to(DEV) for b in bs]


@functools.lru_cache(maxsize=None)
def _pack(C, H):
    from miso_amd import ops
    return ops.DecoderPack(*_weights(C, H))


@functools.lru_cache(maxsize=None)
def _grids(log2, C):
    """(tables, dense twins) on the device, left unchanged"""
    ts = hc.tables(log2, C)
    ds = [hc.dense_from_table(t, d, log2) for t, d in zip(ts, hc.DIMS)]
    assert all(torch.isfinite(t).all() for t in ts)
    return [t.to(DEV) for t in ts], [d.to(DEV).contiguous(memory_format=torch.channels_last_3d) for d in ds]


def _x(n, ac=False):
    x = hc.points(ac).x
    return x[hc.subset(n)] if not ac else x


def _cotangent(n):
    return torch.randn(n, 1, generator=torch.Generator().manual_seed(77 + n))


def _forward_pair(log2, C, H, x, meta):
    """(sdf, mask) of the hash route and of the regular fused route on the dense twins"""
    from miso_amd import ops
    td, dd = _grids(log2, C)
    xd = x.to(DEV)
    got = ops.hash_sdf_fwd_raw(xd, td, meta, hc.DIMS, log2, _pack(C, H), True)
    want = ops.sdf_fwd_raw(xd, dd, meta, _pack(C, H), True)
    torch.cuda.synchronize()
    return got, want


def _same_forward(got, want, n, tag):
    assert got[0].shape == want[0].shape == (n, 1)
    assert torch.equal(_bits(got[0]), _bits(want[0])), f"{tag}: sdf differs from sdf_fwd_raw on the dense twin"
    assert got[1].shape == want[1].shape and got[1].numel() % 64 == 0 and got[1].numel() >= (n + 63) // 64 * 64
    assert torch.equal(got[1].cpu(), want[1].cpu()), f"{tag}: sign words differ"      # all ceil(n / 64) 64 slots


@pytest.mark.parametrize("exact", ARITH)
@pytest.mark.parametrize("C,H", SHAPES)
@pytest.mark.parametrize("log2", hc.LOG2S)
def test_forward_bits_of_the_regular_fused_route_on_the_dense_twin(log2, C, H, exact):
    from miso_amd import ops
    kinds = hc.points().kind
    assert {sc.K[k] for k in ("planes", "faces", "far", "nonfinite")} <= set(kinds[hc.subset(257)].tolist())
    with ops.exact_fp32(exact):
        for n in hc.SIZES + (None,):
            x = _x(n)
            got, want = _forward_pair(log2, C, H, x, _meta())
            _same_forward(got, want, x.shape[0], f"log2 {log2} C {C} H {H} exact {exact} n {n}")
            assert torch.isfinite(got[0]).all()          # (non-finite points decode a zero row)
            if n == 0:
                assert got[0].shape == (0, 1)
            elif n is None:
                assert got[0].std() > 0


@pytest.mark.skipif(bool(os.environ.get("MISO_EXACT_F32")), reason="MISO_EXACT_F32 forces the exact chains: nothing to compare")
@pytest.mark.parametrize("C,H", SHAPES)
def test_decoder_flags_select_the_arithmetic(C, H):
    """the two arithmetics do not agree to the bit: the argument reaches the kernel"""
    from miso_amd import ops
    td, _ = _grids(8, C)
    x = _x(None).to(DEV)
    with ops.exact_fp32(False):
        a, _ = ops.hash_sdf_fwd_raw(x, td, _meta(), hc.DIMS, 8, _pack(C, H), False)
    with ops.exact_fp32(True):
        b, _ = ops.hash_sdf_fwd_raw(x, td, _meta(), hc.DIMS, 8, _pack(C, H), False)
    assert not torch.equal(_bits(a), _bits(b))
    # F_EXACT_F32 in the meta's flags asks for the exact chains as it does on the dense route
    from miso_amd import _lib
    with ops.exact_fp32(False):
        c, _ = ops.hash_sdf_fwd_raw(x, td, _meta(flags=_lib.F_EXACT_F32), hc.DIMS, 8, _pack(C, H), False)
    assert torch.equal(_bits(c), _bits(b))


@pytest.mark.parametrize("exact", ARITH)
@pytest.mark.parametrize("ignore", [(True, False), (False, True)])
@pytest.mark.parametrize("log2", hc.LOG2S)
def test_ignored_levels_contribute_zeros(log2, ignore, exact):
    from miso_amd import ops
    with ops.exact_fp32(exact):
        for C, H in SHAPES:
            x = _x(257)
            meta = _meta(list(ignore))
            got, want = _forward_pair(log2, C, H, x, meta)
            _same_forward(got, want, 257, f"ignore {ignore} log2 {log2} C {C} H {H}")
            full, _ = _forward_pair(log2, C, H, x, _meta())
            assert not torch.equal(_bits(got[0]), _bits(full[0]))


@pytest.mark.parametrize("exact", ARITH)
def test_other_sampling_flags_keep_the_identity(exact):
    from miso_amd import _lib, ops
    meta = _meta(None, _lib.F_PAD_BORDER | _lib.F_ALIGN_CORNERS)
    with ops.exact_fp32(exact):
        for C, H in SHAPES:
            x = _x(None, ac=True)
            got, want = _forward_pair(8, C, H, x, meta)
            _same_forward(got, want, x.shape[0], f"border/ac C {C} H {H}")
            plain, _ = _forward_pair(8, C, H, x, _meta())
            assert not torch.equal(_bits(got[0]), _bits(plain[0]))


def _table_gradient_checks(x, rows, grads, log2, C, tag, pad="zeros", ac=False):
    """every table gradient against the float64 sum of the kernel's fp32 terms; -> (rows with one term, deepest row)"""
    singles, deepest = 0, 0
    r = rows.detach().cpu()
    for l, (gt, dims) in enumerate(zip(grads, hc.DIMS)):
        ref, mag, m = hc.table_gradient64(hc.index_coords(x, dims, pad, ac), dims, log2, r[:, l * C:(l + 1) * C].numpy(), C,
                                          gt.shape[0])
        got = gt.detach().cpu().double().numpy()
        assert np.isfinite(got).all()
        worst = np.abs(got - ref) - m[:, None] * hc.U * mag
        assert (worst <= 0).all(), (f"{tag} level {l}: table gradient {worst.max():.3e} beyond m 2^-24 sum|terms| at row "
                                    f"{int(np.argmax(worst.max(1)))} (m = {int(m[np.argmax(worst.max(1))])})")
        one = m == 1
        assert np.array_equal(got[one], ref[one]), f"{tag} level {l}: a row with one contribution is not exact"
        assert not got[m == 0].any(), f"{tag} level {l}: a row no corner maps to was written"
        singles, deepest = singles + int(one.sum()), max(deepest, int(m.max()))
    return singles, deepest


@pytest.mark.parametrize("exact", ARITH)
@pytest.mark.parametrize("C,H", SHAPES)
@pytest.mark.parametrize("log2", hc.LOG2S)
def test_backward_by_composition(log2, C, H, exact):
    from miso_amd import ops
    td, dd = _grids(log2, C)
    pack, meta = _pack(C, H), _meta()
    with ops.exact_fp32(exact):
        for n in (1, 63, 65, 257, None):
            tag = f"log2 {log2} C {C} H {H} exact {exact} n {n}"
            x = _x(n)
            xd, g = x.to(DEV), _cotangent(x.shape[0]).to(DEV)
            _, mask = ops.hash_sdf_fwd_raw(xd, td, meta, hc.DIMS, log2, pack, True)
            gx, grads, rows = ops.hash_sdf_bwd_raw(xd, td, meta, hc.DIMS, log2, pack, g, mask, True, [True, True])
            # the decoder chain: the rows of the dense route from the same sign words
            _, _, rows_d = ops.sdf_bwd_rows_raw(xd, dd, meta, pack, g, mask, False, [False, False])
            assert rows.shape == (x.shape[0], 2 * C) and torch.equal(_bits(rows), _bits(rows_d)), tag
            assert rows.any()
            # grad_x: the hash encode's backward over those rows
            gx_e, none = ops.hash_encode_bwd_raw(xd, td, meta, hc.DIMS, log2, rows, True, [False, False])
            assert none == [None, None] and gx.shape == (x.shape[0], 3) and torch.equal(_bits(gx), _bits(gx_e)), tag
            singles, deepest = _table_gradient_checks(x, rows, grads, log2, C, tag)
            if n == 1:
                assert singles > 0
            elif n is None:
                assert deepest >= 8 and gx.any()
            # without grad_x: None, and the same table gradients (to the order of the atomics)
            gx2, grads2, rows2 = ops.hash_sdf_bwd_raw(xd, td, meta, hc.DIMS, log2, pack, g, mask, False, [True, True])
            assert gx2 is None and torch.equal(_bits(rows2), _bits(rows))
            _table_gradient_checks(x, rows2, grads2, log2, C, tag + " need_x=False")
            # no table gradient asked: none allocated, grad_x as before
            gx3, grads3, _ = ops.hash_sdf_bwd_raw(xd, td, meta, hc.DIMS, log2, pack, g, mask, True, [False, False])
            assert grads3 == [None, None] and torch.equal(_bits(gx3), _bits(gx))
            # one level asked: the other stays None
            _, grads4, _ = ops.hash_sdf_bwd_raw(xd, td, meta, hc.DIMS, log2, pack, g, mask, False, [False, True])
            assert grads4[0] is None and grads4[1].any()
    torch.cuda.synchronize()
    assert all(torch.equal(a.cpu(), b) for a, b in zip(td, hc.tables(log2, C)))      # the tables were only read


def test_backward_of_an_empty_batch():
    from miso_amd import ops
    td, _ = _grids(6, 4)
    x = torch.zeros(0, 3, device=DEV)
    sdf, mask = ops.hash_sdf_fwd_raw(x, td, _meta(), hc.DIMS, 6, _pack(4, 64), True)
    gx, grads, rows = ops.hash_sdf_bwd_raw(x, td, _meta(), hc.DIMS, 6, _pack(4, 64), torch.zeros(0, 1, device=DEV), mask, True,
                                           [True, True])
    assert sdf.shape == (0, 1) and gx.shape == (0, 3) and rows.shape == (0, 8) and not any(g.any() for g in grads)


@pytest.mark.parametrize("exact", ARITH)
@pytest.mark.parametrize("C,H", SHAPES)
def test_autograd(C, H, exact):
    from miso_amd import ops
    log2 = 8
    td, _ = _grids(log2, C)
    pack, meta = _pack(C, H), _meta()
    x = _x(257)
    g = _cotangent(257).to(DEV)
    with ops.exact_fp32(exact):
        sdf_raw, mask = ops.hash_sdf_fwd_raw(x.to(DEV), td, meta, hc.DIMS, log2, pack, True)
        gx, _, rows = ops.hash_sdf_bwd_raw(x.to(DEV), td, meta, hc.DIMS, log2, pack, g, mask, True, [False, False])
        xr = x.to(DEV).requires_grad_(True)
        tr = [t.clone().requires_grad_(True) for t in td]
        out = ops.hash_sdf_fused(xr, tr, meta, hc.DIMS, log2, pack)
        assert out.requires_grad and torch.equal(_bits(out), _bits(sdf_raw))
        out.backward(g)
        assert torch.equal(_bits(xr.grad), _bits(gx))
        _table_gradient_checks(x, rows, [t.grad for t in tr], log2, C, f"autograd C {C} H {H}")
        # under no_grad: the forward alone, no sign words kept
        with torch.no_grad():
            assert torch.equal(_bits(ops.hash_sdf_fused(xr, tr, meta, hc.DIMS, log2, pack)), _bits(sdf_raw))
        # tables alone
        out = ops.hash_sdf_fused(x.to(DEV), tr, meta, hc.DIMS, log2, pack)
        gts = torch.autograd.grad(out, tr, g)
        _table_gradient_checks(x, rows, gts, log2, C, f"autograd tables only C {C} H {H}")


def test_no_double_backward_and_no_trainable_decoder():
    from miso_amd import ops
    td, _ = _grids(8, 4)
    ts = [t.clone().requires_grad_(True) for t in td]
    pack, meta = _pack(4, 64), _meta()
    x = _x(65).to(DEV).requires_grad_(True)
    out = ops.hash_sdf_fused(x, ts, meta, hc.DIMS, 8, pack)
    (gx,) = torch.autograd.grad(out.sum(), x, create_graph=True)
    assert gx.requires_grad
    with pytest.raises(ops.NoDoubleBackward, match="no second backward"):
        gx.square().sum().backward()
    with ops.coordinate_gradient_only():
        out = ops.hash_sdf_fused(x, ts, meta, hc.DIMS, 8, pack)
        gx2, gt = torch.autograd.grad(out.sum(), [x, ts[0]], create_graph=True, allow_unused=True)
    assert torch.equal(gx2.detach(), gx.detach()) and gt is None
    trainable = ops.DecoderPack(*_weights(4, 64, True))
    assert trainable.trainable()
    with pytest.raises(ops.NotCovered, match="frozen decoder"):
        ops.hash_sdf_fused(x, ts, meta, hc.DIMS, 8, trainable)


@pytest.mark.parametrize("exact", ARITH)
def test_points_outside_and_nan_decode_a_zero_row_and_touch_no_table(exact):
    from miso_amd import ops
    pts = hc.points()
    far = (pts.kind == sc.K["far"]) | (pts.kind == sc.K["nonfinite"])
    x = pts.x[far]
    assert x.shape[0] >= 12 and not torch.isfinite(x).all()
    g = torch.ones(x.shape[0], 1, device=DEV)
    with ops.exact_fp32(exact):
        for log2 in hc.LOG2S:
            for C, H in SHAPES:
                td, dd = _grids(log2, C)
                got, want = _forward_pair(log2, C, H, x, _meta())
                _same_forward(got, want, x.shape[0], f"outside log2 {log2} C {C} H {H}")
                # ... which is the decoder's value on a zero feature row: one number, and the one of a zero table
                zero = [torch.zeros_like(t) for t in td]
                z, _ = ops.hash_sdf_fwd_raw(_x(1).to(DEV), zero, _meta(), hc.DIMS, log2, _pack(C, H), False)
                assert torch.isfinite(z).all() and torch.equal(_bits(got[0]), _bits(z.expand(x.shape[0], 1)))
                gx, grads, rows = ops.hash_sdf_bwd_raw(x.to(DEV), td, _meta(), hc.DIMS, log2, _pack(C, H), g, got[1], True,
                                                       [True, True])
                assert rows.any() and not gx.any() and not any(t.any() for t in grads)
        # a poisoned table: nothing of it reaches points that have no corner in range
        nan = [torch.full_like(t, float("nan")) for t in _grids(6, 4)[0]]
        s, _ = ops.hash_sdf_fwd_raw(x.to(DEV), nan, _meta(), hc.DIMS, 6, _pack(4, 64), False)
        assert torch.isfinite(s).all()


@pytest.mark.parametrize("exact", ARITH)
@pytest.mark.parametrize("C,H", ((4, 64), (8, 64)))
def test_batches_past_the_block_cap_where_the_persistent_waves_loop(C, H, exact):
    """512 blocks of four wavefronts take 131 072 points in one trip each; 65 more and some wavefronts take a second
    chunk, the last of them a partial one.  Forward bits, d-feat rows and grad_x by the same identities as above."""
    from miso_amd import ops
    n, log2 = 512 * 4 * 64 + 65, 8
    b = torch.tensor(sc.BOUNDS[hc.BOUND], dtype=torch.float32)
    gen = torch.Generator().manual_seed(5)
    x = b[:, 0] + (b[:, 1] - b[:, 0]) * (torch.rand(n, 3, generator=gen) * 1.1 - 0.05)      # a few outside the bound
    td, dd = _grids(log2, C)
    pack, meta = _pack(C, H), _meta()
    with ops.exact_fp32(exact):
        got, want = _forward_pair(log2, C, H, x, meta)
        _same_forward(got, want, n, f"n {n} C {C} H {H}")
        xd, g = x.to(DEV), _cotangent(n).to(DEV)
        gx, none, rows = ops.hash_sdf_bwd_raw(xd, td, meta, hc.DIMS, log2, pack, g, got[1], True, [False, False])
        _, _, rows_d = ops.sdf_bwd_rows_raw(xd, dd, meta, pack, g, got[1], False, [False, False])
        gx_e, _ = ops.hash_encode_bwd_raw(xd, td, meta, hc.DIMS, log2, rows, True, [False, False])
    assert none == [None, None] and torch.equal(_bits(rows), _bits(rows_d)) and torch.equal(_bits(gx), _bits(gx_e))
    assert gx[-65:].any() and rows[-65:].any()
