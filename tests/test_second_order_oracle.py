"""Every output of every second-backward path (gridsample_grad2.grad2_3d: encode_bwd2_kernel, encode_bwd2_lean_kernel,
their tile-ordered forms, miso_grad_pull_dx) against fp64 oracles that share none of the kernels' arithmetic:
oracle.grid_sample_bwd2_aten (exact ATen calls and their differences within a cell) on FD-safe points, the fp64
restatement oracle.trilinear_bwd2 (ATen's floor and set-grad conventions) on lattice planes, faces and clip limits.
gg_out, g_x and each level's grid gradient are compared separately.

The oracle is evaluated at the kernel's own fp32 index coordinate (the normalisation replayed in fp32 with the
kernel's operation order, then carried to fp64 exactly): a point one rounding away from a cell plane is then in the
same cell on both sides, and what is measured is the arithmetic, not where the point rounded to.

Tolerances
----------
* per point (gg_out, g_x): max |kernel - fp64| <= 4 x max |fp32 restatement - fp64| on the same inputs, floored at
  1e-6 x max |fp64|;
* grid gradient, per entry: |kernel - fp64| <= 2e-5 A + 1e-12, A the same gradient with every term made positive
  (|gout| |ggx| over each corner a point reaches, |d w| <= 1 in index units): a single wrong contribution can not hide
  inside a large sum.
"""
import pytest
import torch

from oracle import ref_torch as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32
F64 = torch.float64


# --------------------------------------------------------------------------- #
# Oracle at the kernel's coordinates
# --------------------------------------------------------------------------- #
# (the kernel's fp32 normalisation and index coordinate, shared with tests/test_pose_jacobian_oracle.py)
_index32 = R.index32
_norm32 = R.norm32


def _xn64_at_kernel_index(xn32, sizes_xyz, ac):
    """fp64 normalised coordinates whose fp64 unnormalisation is the kernel's fp32 index coordinate."""
    cols = []
    for a, s in enumerate(sizes_xyz):
        i = _index32(xn32[:, a], s, ac).double()
        if ac:
            cols.append(xn32[:, a].double() if s == 1 else i * 2 / (s - 1) - 1)
        else:
            cols.append((2 * i + 1) / s - 1)
    return torch.stack(cols, 1)


def _abs_bound(shape, xn64, gout, ggx_n, pad, ac):
    """A of the module docstring for one level: sum over the points reaching a corner of |gout| sum_a |ggx_a d i_a/d xn_a|
    (|d w / d i_a| <= 1 within a cell; zero on an axis the border clip holds)."""
    _, c, d, h, w = shape
    A = torch.zeros(c, d * h * w, dtype=F64)
    if ggx_n is None or xn64.shape[0] == 0:
        return A.reshape(shape)
    s = torch.zeros(xn64.shape[0], dtype=F64)
    idx = []
    for a, size in enumerate((w, h, d)):
        i = R._unnormalize(xn64[:, a], size, ac)
        m = torch.full_like(i, (size - 1) / 2 if ac else size / 2)
        if pad == "border":
            m = torch.where((i <= 0) | (i >= size - 1), torch.zeros_like(m), m)
            i = i.clamp(0, size - 1)
        s += ggx_n[:, a].abs() * m
        idx.append(torch.floor(i).clamp(-2, size + 1).long())
    val = gout.abs() * s[:, None]                                   # (N,C)
    for k in range(8):
        dx, dy, dz = k & 1, (k >> 1) & 1, k >> 2
        xi, yi, zi = idx[0] + dx, idx[1] + dy, idx[2] + dz
        inb = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h) & (zi >= 0) & (zi < d)
        lin = ((zi * h + yi) * w + xi)[inb]
        A.index_add_(1, lin, val[inb].t())
    return A.reshape(shape)


def _level_oracle(f64, xn64, gout, ggx_n, ggf, pad, ac):
    """(gg_out, g_x per normalised unit, g_feature) in fp64: ATen differences on FD-safe points, the restatement on the
    others."""
    _, c, d, h, w = f64.shape
    safe = R.fd_safe(xn64, (w, h, d), ac)
    n = xn64.shape[0]
    gg, gx, gf = torch.zeros(n, c, dtype=F64), torch.zeros(n, 3, dtype=F64), torch.zeros_like(f64)
    for sel, fd in ((safe, True), (~safe, False)):
        if not sel.any():
            continue
        e = None if ggx_n is None else ggx_n[sel]
        if fd:
            r = R.grid_sample_bwd2_aten(f64, xn64[sel], gout[sel], e, ggf, pad, ac)
        else:
            r = R.trilinear_bwd2(f64, xn64[sel], gout[sel], e, ggf, ac, pad)
        gg[sel], gx[sel] = r[0], r[1]
        gf += r[2]
    return gg, gx, gf


def _check_points(what, got, ref, ref32):
    got = got.detach().double().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite output at a finite point"
    scale = ref.abs().max().item()
    bar = max(4 * (ref32.double() - ref).abs().max().item(), 1e-6 * scale)
    err = (got - ref).abs().max().item()
    assert err <= bar, f"{what}: max |kernel - fp64| = {err:.3e} > {bar:.3e} (scale {scale:.3e})"


def _check_grid(what, got, ref, A):
    got = got.detach().double().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite grid gradient"
    excess = (got - ref).abs() - (2e-5 * A + 1e-12)
    assert excess.max().item() <= 0, \
        f"{what}: {int((excess > 0).sum())} entries beyond 2e-5 A (worst |d| = {(got - ref).abs().max().item():.3e})"


# --------------------------------------------------------------------------- #
# Point sets
# --------------------------------------------------------------------------- #
def _uniform_safe(n, sizes_list, ac, lo, hi, g):
    """Uniform normalised points in [lo, hi]^3, redrawn until 1e-3 index units from every plane of every level."""
    out = torch.empty(0, 3, dtype=F64)
    while out.shape[0] < n:
        x = (torch.rand(2 * n, 3, generator=g, dtype=F64) * (hi - lo) + lo).float().double()
        ok = torch.ones(x.shape[0], dtype=torch.bool)
        for s in sizes_list:
            ok &= R.fd_safe(x, s, ac, margin=2e-3)
        out = torch.cat([out, x[ok]])
    return out[:n]


def _special_points(sizes_xyz, ac, n_lattice, g):
    """Lattice vertices, edge and plane midpoints, both faces and half a cell outside (half-integer index coordinates
    from -1 to size: dyadic for these sizes, exact in fp32); exactly on the faces; one fp32 ulp inside and outside
    them; the align_corners=False zero ramp; 1e9 outside."""
    cols = []
    for s in sizes_xyz:
        i = torch.randint(-2, 2 * s + 1, (n_lattice,), generator=g).double() / 2
        cols.append(i * 2 / max(s - 1, 1) - 1 if ac else (2 * i + 1) / s - 1)
    lat = torch.stack(cols, 1)
    inner = torch.rand(64, 3, generator=g, dtype=F64) * 1.6 - 0.8
    one = torch.tensor(1.0, dtype=F32)
    ulp_in = torch.nextafter(one, torch.tensor(0.0)).double().item()
    ulp_out = torch.nextafter(one, torch.tensor(2.0)).double().item()
    sets = [lat]
    for a in range(3):
        for v in (-1.0, 1.0, -ulp_in, ulp_in, -ulp_out, ulp_out, 1e9, -1e9):
            p = inner[:8].clone()
            p[:, a] = v
            sets.append(p)
        ramp = inner[8:24].clone()              # between the face and half a cell outside
        ramp[:, a] = -1 - torch.rand(16, generator=g, dtype=F64) / sizes_xyz[a]
        sets.append(ramp)
    return torch.cat(sets).float().double()


_CACHE = {}


def _remember(key, value, keep=4):
    """Oracles are computed once per module and input set; the few most recent stay (a cfg-5 level gradient in fp64
    is 150 MB)."""
    while len(_CACHE) >= keep:
        _CACHE.pop(next(iter(_CACHE)))
    _CACHE[key] = value


# --------------------------------------------------------------------------- #
# Drop-in form: cuda_gridsample.grid_sample_3d, all four modes
# --------------------------------------------------------------------------- #
MODES = [(pad, ac) for pad in ("zeros", "border") for ac in (False, True)]
LAYOUTS = ["ncdhw3", "cl4", "cl8", "depth1"]


def _dropin_case(pad, ac, layout, seed):
    g = torch.Generator().manual_seed(seed)
    c = {"ncdhw3": 3, "cl4": 4, "cl8": 8, "depth1": 3}[layout]
    if layout == "depth1":                       # the grid_sample_2d route (compat.py): a depth-1 volume at z = 0
        sizes = (17, 9, 1) if ac else (16, 8, 1)
    else:
        sizes = (17, 9, 5) if ac else (16, 8, 4)
    w, h, d = sizes
    f = torch.randn(1, c, d, h, w, generator=g)
    # (a depth-1 volume samples at z = 0, on a plane: every point goes to the restatement; the depth-4 stand-in only
    # keeps the uniform draw from rejecting all of them)
    safe_sizes = (w, h, 4) if layout == "depth1" else sizes
    x = torch.cat([_uniform_safe(700, [safe_sizes], ac, -1.3, 1.3, g), _special_points(sizes, ac, 300, g)])
    if layout == "depth1":
        x[:, 2] = 0.0
    n = x.shape[0]
    gout = torch.randn(n, c, generator=g)
    ggx = torch.randn(n, 3, generator=g)
    ggf = torch.randn(f.shape, generator=g) * 0.5
    return f, x.float(), gout, ggx, ggf, sizes


def _dropin_kernel(f, x32, gout, ggx, ggf, pad, ac, channels_last, want_input):
    fd = f.to(DEV)
    if channels_last:
        fd = fd.contiguous(memory_format=torch.channels_last_3d)
    fd.requires_grad_(True)
    n = x32.shape[0]
    grid = x32.to(DEV).reshape(1, n, 1, 1, 3).requires_grad_(True)
    from miso_amd import ops
    out = ops.grid_sample_3d(fd, grid, padding_mode=pad, align_corners=ac)
    go = gout.t().reshape(1, -1, n, 1, 1).to(DEV).requires_grad_(True)
    gi, gg = torch.autograd.grad(out, [fd, grid], go, create_graph=True)
    s = 0
    if ggx is not None:
        s = s + (gg.reshape(n, 3) * ggx.to(DEV)).sum()
    if ggf is not None:
        s = s + (gi * ggf.to(DEV)).sum()
    wrt = [go, grid] + ([fd] if want_input else [])
    r = torch.autograd.grad(s, wrt, allow_unused=True)
    gg_out = r[0][0].reshape(-1, n).t()
    g_x = r[1].reshape(n, 3)
    g_in = None
    if want_input:       # (no cotangent of the grid gradient: the second backward hands the input no gradient)
        g_in = torch.zeros_like(fd) if r[2] is None else r[2]
    return gg_out, g_x, g_in


# MISO_ENCODE_NO_LEAN selects between the two VEC4 kernels only: NCDHW and depth-1 (C = 3) run the scalar kernel once
DROPIN_FORMS = [(layout, form) for layout in LAYOUTS
                for form in (("lean", "weight") if layout.startswith("cl") else ("scalar",))]


def _dropin_oracle(pad, ac, layout, cot):
    """The fp64 oracle, the fp32 restatement and A of one drop-in case, once per module (the lean and the weight form
    of a layout share them)."""
    key = ("dropin", pad, ac, layout, cot)
    if key not in _CACHE:
        f, x32, gout, ggx, ggf, sizes = _dropin_case(pad, ac, layout, seed=4 * LAYOUTS.index(layout) + MODES.index((pad, ac)))
        e = ggx if cot != "ggf" else None
        gg = ggf if cot != "ggx" else None
        xn64 = _xn64_at_kernel_index(x32, sizes, ac)
        e64 = None if e is None else e.double()
        ref = _level_oracle(f.double(), xn64, gout.double(), e64, None if gg is None else gg.double(), pad, ac)
        r32 = R.trilinear_bwd2(f, x32, gout, e, gg, ac, pad)
        A = _abs_bound(f.shape, xn64, gout.double(), e64, pad, ac)
        _remember(key, ((f, x32, gout, e, gg), ref, r32, A))
    return _CACHE[key]


@pytest.mark.parametrize("pad,ac", MODES)
@pytest.mark.parametrize("layout,form", DROPIN_FORMS)
def test_dropin_second_backward_vs_fp64(pad, ac, layout, form, monkeypatch):
    """gg_out, grad of the grid and grad of the input of the second backward of ops.grid_sample_3d; the grad output
    requires grad, so gg_out is formed.  NCDHW runs the scalar kernels, channels-last C = 4 / 8 the VEC4 ones (the lean
    lerp-tree kernel where the launch scatters no grid gradient: without the input among the wanted gradients, or
    with the grid-gradient cotangent only; MISO_ENCODE_NO_LEAN=1 the weight form)."""
    if form == "weight":
        monkeypatch.setenv("MISO_ENCODE_NO_LEAN", "1")
    for cot in ("ggx", "ggf", "both"):
        (f, x32, gout, e, gg), ref, r32, A = _dropin_oracle(pad, ac, layout, cot)
        for want_input in (True, False):
            got = _dropin_kernel(f, x32, gout, e, gg, pad, ac, layout.startswith("cl"), want_input)
            tag = f"{pad}/ac={ac}/{layout}/{form}/{cot}/input={want_input}"
            _check_points(tag + " gg_out", got[0], ref[0], r32[0])
            _check_points(tag + " g_x", got[1], ref[1], r32[1])
            if want_input:
                _check_grid(tag + " g_input", got[2], ref[2], A)


# --------------------------------------------------------------------------- #
# Encode form: ops.encode_bwd2_raw, the product convention (zeros, align_corners=False, metres)
# --------------------------------------------------------------------------- #
SHAPES = {     # level sizes (x, y, z) and bound of test_split_precision.SHAPES
    "cfg1": ([(64, 64, 64)], [[-1.0, 1.0]] * 3),
    "cfg2": ([(32, 32, 32), (64, 64, 64), (128, 128, 128)], [[-1.0, 1.0]] * 3),
    "cfg2_half": ([(16, 16, 16), (32, 32, 32), (64, 64, 64)], [[-1.0, 1.0]] * 3),     # (a cheaper oracle)
    "cfg3": ([(40, 20, 40), (200, 100, 200)], [[-10.0, 10.0], [-5.0, 5.0], [-10.0, 10.0]]),
    "cfg5": ([(10, 30, 30), (20, 60, 60), (40, 120, 120), (80, 240, 240)], [[-30.0, 30.0], [-30.0, 30.0], [-5.0, 15.0]]),
}


def _encode_inputs(shape, C, n, seed, special=True):
    levels, bound = SHAPES[shape]
    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn(1, C, z, y, x, generator=g) for (x, y, z) in levels]
    sizes = [tuple(s) for s in levels]
    xn = _uniform_safe(n, sizes, False, -1.1, 1.1, g)
    if special:
        dyadic = all(b == [-1.0, 1.0] for b in bound)
        sp = _special_points(sizes[-1], False, 200 if dyadic else 0, g)
        xn = torch.cat([xn[: max(n - sp.shape[0], 0)], sp])[:n] if n > sp.shape[0] else xn
    b = torch.tensor(bound, dtype=F64)
    x = R.denormalize_coordinates(xn, b).float()
    on_face = (xn.abs() == 1).any(1)
    x[on_face] = torch.where(xn[on_face] == 1, b[:, 1].float(), torch.where(xn[on_face] == -1, b[:, 0].float(), x[on_face]))
    gout = torch.randn(n, C * len(levels), generator=g)
    ggx = torch.randn(n, 3, generator=g)
    ggf = [torch.randn(f.shape, generator=g) * 0.5 for f in feats]
    return feats, bound, x, gout, ggx, ggf


def _encode_oracle(feats, bound, x32, gout, ggx, ggf, ignore):
    """fp64 oracle and fp32 restatement of encode_bwd2_raw's three outputs; A per level."""
    xn32 = _norm32(x32, bound)
    fin = torch.isfinite(x32).all(1)
    sc = 2 / (torch.tensor(bound, dtype=F64)[:, 1] - torch.tensor(bound, dtype=F64)[:, 0])
    n = x32.shape[0]
    gg, gx, gf, A = torch.zeros(n, gout.shape[1], dtype=F64), torch.zeros(n, 3, dtype=F64), [], []
    gg32, gx32 = torch.zeros(n, gout.shape[1]), torch.zeros(n, 3)
    c0 = 0
    for l, f in enumerate(feats):
        c = f.shape[1]
        if ignore[l]:
            gf.append(torch.zeros_like(f, dtype=F64))
            A.append(torch.zeros_like(f, dtype=F64))
            c0 += c
            continue
        sizes = (f.shape[4], f.shape[3], f.shape[2])
        xn64 = _xn64_at_kernel_index(xn32[fin], sizes, False)
        e = None if ggx is None else ggx[fin].double() * sc
        g_l = None if ggf is None else ggf[l]
        r = _level_oracle(f.double(), xn64, gout[fin, c0:c0 + c].double(), e, None if g_l is None else g_l.double(),
                          "zeros", False)
        gg[fin, c0:c0 + c] = r[0]
        gx[fin] += r[1] * sc
        gf.append(r[2])
        A.append(_abs_bound(f.shape, xn64, gout[fin, c0:c0 + c].double(), e, "zeros", False))
        r32 = R.trilinear_bwd2(f, xn32[fin], gout[fin, c0:c0 + c], None if ggx is None else ggx[fin] * sc.float(),
                               g_l, False, "zeros")
        gg32[fin, c0:c0 + c] = r32[0]
        gx32[fin] += r32[1] * sc.float()
        c0 += c
    return (gg, gx, gf, A), (gg32, gx32)


def _run_raw(feats, bound, x32, gout, ggx, ggf, ignore, layout, path, gout_rows="packed", ggf_layout="same"):
    from miso_amd import ops
    fd = [f.to(DEV) for f in feats]
    if layout == "cl":
        fd = [f.contiguous(memory_format=torch.channels_last_3d) for f in fd]
    meta = ops.GridMeta.from_bound(bound, ignore)
    n, F = gout.shape
    if gout_rows == "packed":
        go = gout.to(DEV)
    elif gout_rows == "ld%4":                         # row stride F + 1
        go = torch.zeros(n, F + 1, device=DEV)[:, :F]
        go.copy_(gout)
    else:                                             # rows 4 bytes off a 16-byte boundary
        go = torch.zeros(n, F + 4, device=DEV)[:, 1:F + 1]
        go.copy_(gout)
    gg_d = None
    if ggf is not None:
        gg_d = []
        for l, t in enumerate(ggf):
            if t is None:
                gg_d.append(None)
                continue
            t = t.to(DEV)
            if ggf_layout == "other":                 # a cotangent in the other layout: the kernel reads a copy
                t = t.contiguous() if layout == "cl" else t.contiguous(memory_format=torch.channels_last_3d)
            elif layout == "cl":
                t = t.contiguous(memory_format=torch.channels_last_3d)
            gg_d.append(t)
    xd = x32.to(DEV)
    need_f = [ggx is not None] * len(fd)
    keep = ops.ENCODE_PULL_MIN_POINTS
    if path in ("unsorted", "sorted"):        # "pull" / "auto": the default choice (the pull from 16384 points)
        ops.ENCODE_PULL_MIN_POINTS = None
    try:
        sb = ops.SortedBatch(n, xd.device).sort(xd, meta) if path == "sorted" else None
        r = ops.encode_bwd2_raw(xd, fd, meta, go, None if ggx is None else ggx.to(DEV), gg_d, True, need_f,
                                sorted_batch=sb)
        torch.cuda.synchronize()
    finally:
        ops.ENCODE_PULL_MIN_POINTS = keep
    return r


ENCODE_CASES = [   # shape, C, layout, path
    ("cfg3", 4, "cl", "unsorted"), ("cfg3", 4, "cl", "sorted"), ("cfg3", 4, "cl", "pull"),
    ("cfg3", 2, "ncdhw", "unsorted"), ("cfg3", 4, "ncdhw", "sorted"),
    ("cfg2", 8, "cl", "sorted"), ("cfg2", 8, "cl", "pull"), ("cfg2", 2, "ncdhw", "unsorted"),
    ("cfg1", 4, "cl", "pull"), ("cfg1", 1, "ncdhw", "sorted"),
    ("cfg5", 1, "ncdhw", "unsorted"), ("cfg5", 4, "cl", "pull"),
]


@pytest.mark.parametrize("shape,C,layout,path", ENCODE_CASES, ids=["-".join(map(str, c)) for c in ENCODE_CASES])
def test_encode_second_backward_vs_fp64(shape, C, layout, path, monkeypatch):
    """encode_bwd2_raw in the product convention on the level shapes of cfg-1/2/3/5: unsorted, with a SortedBatch, and
    on the pull path (n >= ENCODE_PULL_MIN_POINTS: miso_grad_pull_dx forms the grid gradient); cotangents ggx only,
    ggf on every level, ggf on a subset, ggf in the other layout; an ignored level; grad-output rows of stride F + 1 and
    at a 4-byte offset (the non-lean fallback, no pull)."""
    from miso_amd import ops
    n = 20000 if path == "pull" else 3000
    if path == "pull":
        assert n >= ops.ENCODE_PULL_MIN_POINTS
    feats, bound, x, gout, ggx, ggf = _encode_inputs(shape, C, n, seed=len(shape) * 31 + C)
    L = len(feats)
    lib = ops._lib.load()
    calls = []
    real = lib.miso_grad_pull_dx
    monkeypatch.setattr(lib, "miso_grad_pull_dx", lambda *a: (calls.append(1), real(*a))[1])
    ign1 = [True] + [False] * (L - 1) if L > 1 else [False]
    # (tag, oracle: the cotangents' name, ggx, ggf, ignore; grad-output rows, layout of ggf)
    variants = [
        ("ggx", "ggx", ggx, None, [False] * L, "packed", "same"),
        ("ggx+ggf", "ggx+ggf", ggx, ggf, [False] * L, "packed", "same"),
        ("ggf-subset", "ggf0", None, [ggf[0]] + [None] * (L - 1), [False] * L, "packed", "same"),
        ("ggx+ggf-other-layout+ignore", "ggx+ggf", ggx, ggf, ign1, "packed", "other"),
    ]
    if path == "unsorted":
        variants += [("ggx+ggf ld%4", "ggx+ggf", ggx, ggf, [False] * L, "ld%4", "same"),
                     ("ggx+ggf offset4", "ggx+ggf", ggx, ggf, [False] * L, "offset4", "same")]
    for tag, cots, e, gg, ign, rows, ggl in variants:
        key = ("encode", shape, C, n, cots, tuple(ign))       # (the unsorted and sorted paths share n = 3000 inputs)
        if key not in _CACHE:
            _remember(key, _encode_oracle(feats, bound, x, gout, e, gg, ign))
        ref, r32 = _CACHE[key]
        calls.clear()
        gg_out, g_x, g_f = _run_raw(feats, bound, x, gout, e, gg, ign, layout, path, rows, ggl)
        if path == "pull" and e is not None and rows == "packed":
            assert calls, "the pull path did not run"
        what = f"{shape}/C={C}/{layout}/{path}/{tag}"
        _check_points(what + " gg_out", gg_out, ref[0], r32[0])
        _check_points(what + " g_x", g_x, ref[1], r32[1])
        for l in range(L):
            if e is None:
                assert g_f[l] is None
            else:
                _check_grid(f"{what} g_level{l}", g_f[l], ref[2][l], ref[3][l])


@pytest.mark.parametrize("n", [0, 1, 63, 65, 16383, 16384, 70001])
def test_encode_second_backward_batch_sizes(n):
    """Partial wavefronts and workgroups, and both sides of ENCODE_PULL_MIN_POINTS (the default path choice)."""
    feats, bound, x, gout, ggx, ggf = _encode_inputs("cfg2_half", 4, n, seed=n % 97, special=n >= 1000)
    ref, r32 = _encode_oracle(feats, bound, x, gout, ggx, ggf, [False] * 3)
    gg_out, g_x, g_f = _run_raw(feats, bound, x, gout, ggx, ggf, [False] * 3, "cl", "auto")
    assert gg_out.shape == (n, 12) and g_x.shape == (n, 3)
    if n:
        _check_points(f"n={n} gg_out", gg_out, ref[0], r32[0])
        _check_points(f"n={n} g_x", g_x, ref[1], r32[1])
    for l in range(3):
        _check_grid(f"n={n} g_level{l}", g_f[l], ref[2][l], ref[3][l])


def test_sparse_batches_every_path(monkeypatch):
    """At most a few points per cell, so that each grid entry holds one or two contributions: per path."""
    from miso_amd import ops
    g = torch.Generator().manual_seed(77)
    feats = [torch.randn(1, 4, 40, 80, 80, generator=g)]
    bound = [[-1.0, 1.0]] * 3
    n = 16384
    xn = _uniform_safe(n, [(80, 80, 40)], False, -1.0, 1.0, g)
    x = xn.float()
    gout = torch.randn(n, 4, generator=g)
    ggx = torch.randn(n, 3, generator=g)
    ggf = [torch.randn(feats[0].shape, generator=g)]
    ref, r32 = _encode_oracle(feats, bound, x, gout, ggx, ggf, [False])
    for path in ("unsorted", "sorted", "pull"):
        gg_out, g_x, g_f = _run_raw(feats, bound, x, gout, ggx, ggf, [False], "cl", path)
        _check_points(f"sparse/{path} gg_out", gg_out, ref[0], r32[0])
        _check_points(f"sparse/{path} g_x", g_x, ref[1], r32[1])
        _check_grid(f"sparse/{path} g_level0", g_f[0], ref[2][0], ref[3][0])


@pytest.mark.parametrize("path", ["unsorted", "sorted", "pull"])
def test_non_finite_points_change_nothing_else(path):
    """NaN and +-inf points added to a batch: the other points' outputs are the same bits (unsorted) or the same to
    rounding (a binned batch gathers in another order), the grid gradients the same up to atomic-order noise, and every
    finite point's output is finite."""
    feats, bound, x, gout, ggx, ggf = _encode_inputs("cfg3", 4, 17000, seed=5)
    bad = torch.tensor([[float("nan"), 0.0, 0.0], [0.0, float("inf"), 0.0], [0.0, 0.0, float("-inf")],
                        [float("nan")] * 3, [float("inf")] * 3, [1.0, float("-inf"), float("nan")]])
    pos = torch.tensor([0, 5, 999, 4000, 12000, 16999])
    keep = torch.ones(17000 + len(pos), dtype=torch.bool)
    keep[pos + torch.arange(len(pos))] = False
    xb = torch.empty(keep.shape[0], 3)
    xb[keep], xb[~keep] = x, bad
    gob = torch.zeros(keep.shape[0], gout.shape[1])
    gob[keep], gob[~keep] = gout, torch.randn(len(pos), gout.shape[1])
    gxb = torch.zeros(keep.shape[0], 3)
    gxb[keep], gxb[~keep] = ggx, torch.randn(len(pos), 3)
    a = _run_raw(feats, bound, x, gout, ggx, ggf, [False, False], "cl", path)
    b = _run_raw(feats, bound, xb, gob, gxb, ggf, [False, False], "cl", path)
    ref, _ = _encode_oracle(feats, bound, x, gout, ggx, ggf, [False, False])
    for t in (a[0], a[1], b[0][keep.to(DEV)], b[1][keep.to(DEV)]):
        assert torch.isfinite(t).all()
    if path == "unsorted":
        assert torch.equal(a[0], b[0][keep.to(DEV)]) and torch.equal(a[1], b[1][keep.to(DEV)])
    else:
        torch.testing.assert_close(b[0][keep.to(DEV)], a[0], rtol=1e-6, atol=1e-6 * a[0].abs().max().item())
        torch.testing.assert_close(b[1][keep.to(DEV)], a[1], rtol=1e-6, atol=1e-6 * a[1].abs().max().item())
    for l in range(2):
        _check_grid(f"non-finite/{path} g_level{l} (clean batch)", a[2][l], ref[2][l], ref[3][l])
        _check_grid(f"non-finite/{path} g_level{l}", b[2][l], ref[2][l], ref[3][l])


# --------------------------------------------------------------------------- #
# The fused double backward (ops.sdf_fused with create_graph=True: _SdfFusedBackward) against fp64
# --------------------------------------------------------------------------- #
FUSED = {   # level sizes (x, y, z), C, hidden width, bound
    "cfg3": ([(40, 20, 40), (200, 100, 200)], 4, 64, [[-10.0, 10.0], [-5.0, 5.0], [-10.0, 10.0]]),
    "cfg2": ([(32, 32, 32), (64, 64, 64), (128, 128, 128)], 8, 64, [[-1.0, 1.0]] * 3),
}
TIE = 1e-6


def _fused_inputs(shape, n):
    levels, C, H, bound = FUSED[shape]
    gen = torch.Generator().manual_seed(n + len(shape))
    b = torch.tensor(bound, dtype=F32)
    x = b[:, 0] + (b[:, 1] - b[:, 0]) * (torch.rand(n, 3, generator=gen) * 1.04 - 0.02)
    feats = [torch.randn((1, C, z, y, xx), generator=gen) * 3e-2 for (xx, y, z) in levels]
    torch.manual_seed(n)
    lin = [torch.nn.Linear(C * len(levels), H), torch.nn.Linear(H, H), torch.nn.Linear(H, 1)]
    ws = [l.weight.detach().clone() * (8.0 if i == 0 else 1.0) for i, l in enumerate(lin)]  # pre-activations ~ 1
    bs = [l.bias.detach().clone() for l in lin]
    cot = torch.rand(n, 1, generator=gen) + 0.5            # the cotangent of sdf in d sdf / d x
    return x, feats, b, ws, bs, cot


def _eik_loss(sdf, g, keep):
    """Eikonal + |sdf| (grid_opt/loss_isdf.py:96-152,367-377); ReLU-tie and cell-plane points carry no weight."""
    return (keep * (g.norm(dim=1) - 1) ** 2).mean() + (keep * sdf.abs().view(-1)).mean()


def _fused_oracle(x, feats, b, ws, bs, cot):
    """Full fp64 autograd through the any-order restatement (oracle.encode_gather, pinned to the ATen-built oracle and
    to the reference's naive sampler by tests/test_oracle_golden.py) and the MLP: it differentiates the decoder as
    autograd does (ReLU'' = 0), without the fused path's "rows are piecewise constant" argument."""
    xd = x.double().requires_grad_(True)
    fd = [f.double().requires_grad_(True) for f in feats]
    cd = cot.double().requires_grad_(True)
    wd, bd = [w.double() for w in ws], [v.double() for v in bs]
    pre1 = R.encode_gather(fd, b.double(), xd) @ wd[0].T + bd[0]
    pre2 = torch.relu(pre1) @ wd[1].T + bd[1]
    sdf = torch.relu(pre2) @ wd[2].T + bd[2]
    keep = torch.minimum(pre1.detach().abs().min(1).values, pre2.detach().abs().min(1).values) >= TIE
    # and the points within fp32 rounding of a cell plane, where the second derivatives jump and an fp32 evaluation
    # may take the other cell (the kernels' own conventions there are tested above)
    xn = R.normalize_coordinates(x.double(), b.double())
    for f in feats:
        keep &= R.fd_safe(xn, (f.shape[4], f.shape[3], f.shape[2]), False, margin=1e-4)
    keep = keep.double()
    (g,) = torch.autograd.grad(sdf, xd, cd, create_graph=True)
    got = torch.autograd.grad(_eik_loss(sdf, g, keep), fd + [xd, cd])
    return list(got), keep


def _fused_device(exact, x, feats, b, ws, bs, cot, keep):
    from miso_amd import ops
    meta = ops.GridMeta.from_bound(b)
    pack = ops.DecoderPack([w.to(DEV) for w in ws], [v.to(DEV) for v in bs])
    xd = x.to(DEV).requires_grad_(True)
    fd = [f.to(DEV).contiguous(memory_format=torch.channels_last_3d).requires_grad_(True) for f in feats]
    cd = cot.to(DEV).requires_grad_(True)
    with ops.exact_fp32(exact):
        sdf = ops.sdf_fused(xd, fd, meta, pack)
        (g,) = torch.autograd.grad(sdf, xd, cd, create_graph=True)
        got = torch.autograd.grad(_eik_loss(sdf, g, keep.float().to(DEV)), fd + [xd, cd])
    torch.cuda.synchronize()
    return [t.detach().double().cpu() for t in got]


@pytest.mark.parametrize("shape,n", [("cfg3", 300), ("cfg3", 3000), ("cfg3", 70000), ("cfg2", 3000), ("cfg2", 70000)])
def test_fused_double_backward_vs_fp64(shape, n):
    """Gradients of an eikonal + |sdf| loss through ops.sdf_fused with create_graph=True w.r.t. every level, x and the
    sdf cotangent, against fp64, under the exact fp32 decoder chains and the split (bf16x3) ones.  n = 70 000 bins the
    batch (SortedBatch.AUTO_MIN_POINTS).  Bars: the exact form's mean error within 1e-4 of each quantity's scale; the
    split form within 2x the exact form's own max and mean error (the admissibility bar of
    tests/test_split_precision.py)."""
    x, feats, b, ws, bs, cot = _fused_inputs(shape, n)
    ref, keep = _fused_oracle(x, feats, b, ws, bs, cot)
    assert keep.mean() > 0.99
    ex = _fused_device(True, x, feats, b, ws, bs, cot, keep)
    sp = _fused_device(False, x, feats, b, ws, bs, cot, keep)
    names = [f"grad_level{l}" for l in range(len(feats))] + ["grad_x", "grad_sdf_cotangent"]
    report = []
    for what, e, s, r in zip(names, ex, sp, ref):
        assert torch.isfinite(e).all() and torch.isfinite(s).all(), what
        de, ds = (e - r).abs(), (s - r).abs()
        scale = r.abs().max().item()
        report.append(f"{shape} n={n} {what}: exact max {de.max():.3e} mean {de.mean():.3e} | split max {ds.max():.3e} "
                      f"mean {ds.mean():.3e} | scale {scale:.3e}")
        assert scale > 0, report[-1]
        # a wrong or missing term moves the mean error by the order of the scale; a lone outlier common to both forms (a
        # gate within fp32 rounding of a tie) is what the 2x bar below already accepts, as test_split_precision does
        assert de.mean().item() <= 1e-4 * scale, report[-1]
        assert ds.max().item() <= 2.0 * de.max().item() + 1e-7 * scale, report[-1]
        assert ds.mean().item() <= 2.0 * de.mean().item() + 2e-9 * scale, report[-1]
    print("\n".join(report))
