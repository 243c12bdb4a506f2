"""Pin the CPU oracle (oracle/ref_torch.py) against the reference's outputs
captured in tests/golden (tools/make_goldens.py) and against the known-answer
inputs of the reference's own third_party/cuda_gridsample_grad2/test3d.py."""
import numpy as np
import pytest
import torch

import golden_cases as gc
from oracle import ref_torch as R


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _load(name):
    return np.load(gc.golden_path(name))


@pytest.mark.parametrize("name", ["small", "cfg1", "cfg2"])
@pytest.mark.parametrize("impl", ["stock", "gather"])
def test_encode_decode_matches_reference(name, impl):
    if name == "cfg2" and impl == "gather":
        pytest.skip("covered by small/cfg1; cfg2 gather restatement is slow on CPU")
    case = gc.CASES[name]
    g = _load(name)
    feats = [T(f).requires_grad_(True) for f in gc.make_features(case)]
    stab = [T(f) for f in gc.make_stability(case)]
    bound = torch.tensor(case["bound"], dtype=torch.float32)
    ws, bs = R.decoder_params({k: T(v) for k, v in gc.make_decoder(case).items()})
    x = T(gc.make_points(case)).requires_grad_(True)
    n = x.shape[0]
    sdf_t, valid, sign, weight = [T(a) for a in gc.make_targets(case, n)]
    enc = R.encode_stock if impl == "stock" else R.encode_gather
    f = enc(feats, bound, x)
    tol = dict(rtol=0, atol=1e-7) if impl == "stock" else dict(rtol=1e-5, atol=2e-7)
    torch.testing.assert_close(f.detach(), T(g["feats"]), **tol)
    torch.testing.assert_close(enc(stab, bound, x).detach(), T(g["stab"]), rtol=1e-5, atol=1e-6)
    pred = R.mlp_forward(f, ws, bs)
    torch.testing.assert_close(pred.detach(), T(g["sdf"]), rtol=1e-5, atol=1e-6)
    l1 = R.miso_loss_regression(pred, sdf_t, valid, weight, "L1")
    fs = R.miso_loss_free_space(pred, sdf_t, sign, 0.15)
    assert abs(l1.item() - float(g["loss_l1"])) < 1e-6
    assert abs(fs.item() - float(g["loss_fs"])) < 1e-6
    grads = torch.autograd.grad(l1 + 0.1 * fs, feats + [x])
    torch.testing.assert_close(grads[-1], T(g["grad_x"]), rtol=1e-4, atol=1e-7)
    for l in range(case["n_levels"]):
        gl = grads[l].reshape(-1)
        idx = T(g[f"gfeat{l}_idx"])
        torch.testing.assert_close(gl[idx], T(g[f"gfeat{l}_val"]), rtol=1e-4, atol=1e-9)
        assert abs(gl.double().abs().sum().item() - float(g[f"gfeat{l}_abssum"])) \
            <= 1e-4 * float(g[f"gfeat{l}_abssum"])


def test_known_answers_from_reference_test3d():
    """third_party/cuda_gridsample_grad2/test3d.py:17-35 inputs; values
    cross-checked against F.grid_sample (the reference's forward, cuda_gridsample.py:84)."""
    cases = [
        (torch.arange(27, dtype=torch.float64).reshape(1, 1, 3, 3, 3), [0.1, 0.1, 0.1], "border", True),
        (torch.arange(8, dtype=torch.float64).reshape(1, 1, 2, 2, 2), [0.1, 1.1, 0.1], "border", True),
        (torch.arange(27, dtype=torch.float64).reshape(1, 1, 3, 3, 3), [-2.1, 0.1, 0.1], "zeros", True),
        (torch.arange(27, dtype=torch.float64).reshape(1, 1, 3, 3, 3), [-0.95, 0.99, 0.3], "zeros", False),
    ]
    for inp, q, pad, ac in cases:
        xn = torch.tensor([q], dtype=torch.float64)
        a = R.trilinear_gather(inp, xn, align_corners=ac, padding_mode=pad)
        b = R.grid_sample_stock(inp, xn, align_corners=ac, padding_mode=pad)
        torch.testing.assert_close(a, b)
    # arange(27) volume, align_corners=True, centre+0.1 -> 13 + 0.1*(1+3+9)
    v = R.trilinear_gather(cases[0][0], torch.tensor([[0.1, 0.1, 0.1]], dtype=torch.float64), True, "border")
    assert abs(v.item() - (13 + 0.1 * 13)) < 1e-12


@pytest.mark.parametrize("pad", ["zeros", "border"])
@pytest.mark.parametrize("ac", [False, True])
def test_gather_first_derivatives_match_aten(pad, ac):
    torch.manual_seed(0)
    inp = torch.randn(1, 3, 5, 6, 7, dtype=torch.float64, requires_grad=True)
    xn = (torch.rand(200, 3, dtype=torch.float64) * 2.6 - 1.3).requires_grad_(True)
    go = torch.randn(200, 3, dtype=torch.float64)
    a = R.trilinear_gather(inp, xn, ac, pad)
    b = R.grid_sample_stock(inp, xn, ac, pad)
    torch.testing.assert_close(a, b)
    ga = torch.autograd.grad((a * go).sum(), [inp, xn])
    gb = torch.autograd.grad((b * go).sum(), [inp, xn])
    torch.testing.assert_close(ga[0], gb[0])
    torch.testing.assert_close(ga[1], gb[1])


def test_gather_gradgradcheck():
    """Style of test3d.py:37-72: gradcheck + gradgradcheck in fp64, in- and out-of-bounds."""
    torch.manual_seed(1)
    inp = torch.randn(1, 2, 4, 3, 5, dtype=torch.float64, requires_grad=True)
    xn = (torch.rand(12, 3, dtype=torch.float64) * 2.4 - 1.2).requires_grad_(True)
    fn = lambda i, g: R.trilinear_gather(i, g, False, "zeros")
    assert torch.autograd.gradcheck(fn, (inp, xn))
    assert torch.autograd.gradgradcheck(fn, (inp, xn))


def test_so3_and_pose_goldens_parity_unpinned_vs_pytorch3d():
    """NOT a pin against pytorch3d (absent from the image, an unpinned git dependency upstream): the golden came from
    the reference run on tools/ref_shims/pytorch3d, a restatement of the same recalled formula as oracle.so3_exp_map
    and miso_amd.so3 -- three copies, so a shared mistake would be invisible here.  The independent check is
    test_so3_exp_map_equals_the_matrix_exponential below."""
    g = _load("so3")
    R0 = T(gc.rodrigues([0.2, 0.1, -0.3]).astype(np.float32))
    t0 = torch.tensor([[1.0], [2.0], [3.0]])
    for i, w in enumerate([[0.0, 0.0, 0.0], [1e-3, -2e-3, 5e-4], [0.3, -0.2, 0.1], [1.2, 0.4, -0.9]]):
        dr = torch.tensor([w], dtype=torch.float32, requires_grad=True)
        dt = torch.tensor([[0.1], [-0.2], [0.3]], dtype=torch.float32)
        Rn, tn = R.apply_pose_correction(R0, t0, dr, dt)
        wgt = torch.arange(9, dtype=torch.float32).reshape(3, 3) / 10
        (Rn * wgt).sum().backward()
        torch.testing.assert_close(Rn.detach(), T(g[f"R_{i}"]), rtol=0, atol=1e-7)
        torch.testing.assert_close(tn, T(g[f"t_{i}"]))
        torch.testing.assert_close(dr.grad, T(g[f"gdr_{i}"]), rtol=1e-5, atol=1e-6)


def test_so3_exp_map_equals_the_matrix_exponential():
    """Independent of the recalled Rodrigues formula: so3_exp_map(w) = expm(hat(w)) (torch.linalg.matrix_exp, a Pade /
    Taylor evaluation) for |w|^2 >= eps = 1e-4, where the angle clamp is inactive -- values and the gradient w.r.t. w,
    for the oracle's restatement and the product's (miso_amd.so3, plain torch, runs on CPU).  Below the clamp the
    function is by construction NOT the exponential (theta is held at 0.01): there the first-order behaviour is
    checked instead: R(w) = I + (sin .01 / .01) hat(w) + O(|w|^2)."""
    from miso_amd import so3 as P
    for mod in (R, P):
        for w in ([0.3, -0.2, 0.1], [1.2, 0.4, -0.9], [0.02, 0.0, 0.0], [-2.0, 1.0, 2.0], [0.006, -0.006, 0.006]):
            v = torch.tensor([w], dtype=torch.float64, requires_grad=True)
            assert float((v * v).sum()) >= 1e-4
            E = mod.so3_exp_map(v)[0]
            M = torch.linalg.matrix_exp(mod.hat(v)[0])
            torch.testing.assert_close(E, M, rtol=0, atol=1e-9)
            wgt = torch.arange(9, dtype=torch.float64).reshape(3, 3) / 10
            ga, = torch.autograd.grad((E * wgt).sum(), v, retain_graph=True)
            gb, = torch.autograd.grad((M * wgt).sum(), v)
            torch.testing.assert_close(ga, gb, rtol=0, atol=1e-8)
            torch.testing.assert_close(E @ E.T, torch.eye(3, dtype=torch.float64), rtol=0, atol=1e-12)
        # hat: [v]_x u = v x u
        a, b = torch.tensor([[0.3, -1.2, 0.7]], dtype=torch.float64), torch.tensor([0.5, 0.1, -0.4], dtype=torch.float64)
        torch.testing.assert_close(mod.hat(a)[0] @ b, torch.linalg.cross(a[0], b))
        # inside the clamp: linear in w with slope sin(0.01) / 0.01
        v = torch.tensor([[2e-3, -1e-3, 5e-4]], dtype=torch.float64)
        lin = torch.eye(3, dtype=torch.float64) + (np.sin(0.01) / 0.01) * mod.hat(v)[0]
        assert (mod.so3_exp_map(v)[0] - lin).abs().max().item() < 3e-6      # the K^2 term: |w|^2 / 2


def test_pairwise_latent_matches_reference():
    g = _load("atlas")
    c = gc.ATLAS
    subs = gc.atlas_inputs()
    bound = torch.tensor(c["bound"], dtype=torch.float32)
    # cached coordinates: voxel centres whose multi-level feature norm > 1e-5 (grid_atlas.py:565-579)
    coords = {}
    for s, sub in enumerate(subs):
        feats = [T(f) for f in sub["features"]]
        for l, f in enumerate(feats):
            _, _, nz, ny, nx = f.shape
            ax = [2 * torch.linspace(0.5 / n, 1 - 0.5 / n, n) - 1 for n in (nx, ny, nz)]
            zz, yy, xx = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
            pn = torch.stack([xx, yy, zz], -1).reshape(-1, 3)
            p = R.denormalize_coordinates(pn, bound)
            fe = R.encode_stock(feats, bound, p)
            keep = torch.linalg.norm(fe, dim=1) > 1e-5
            coords[(s, l)] = p[keep]
            assert coords[(s, l)].shape[0] == int(g[f"ncoords_s{s}_l{l}"])
    for (a, b) in [(0, 1), (0, 2), (1, 2)]:
        for l in range(c["n_levels"]):
            for lt in ("L2", "L1"):
                prm = {}
                for s in (a, b):
                    prm[s] = (T(subs[s]["dr"]).clone().requires_grad_(True),
                              T(subs[s]["dt"]).clone().requires_grad_(True))
                Ra, ta = R.apply_pose_correction(T(subs[a]["R"]), T(subs[a]["t"]), *prm[a])
                Rb, tb = R.apply_pose_correction(T(subs[b]["R"]), T(subs[b]["t"]), *prm[b])
                loss = R.pairwise_latent_loss([T(f) for f in subs[a]["features"]], bound,
                                              [T(f) for f in subs[b]["features"]], bound,
                                              coords[(a, l)], Ra, ta, Rb, tb, l, c["fdim"],
                                              align_loss=lt)
                key = f"latent_{a}_{b}_l{l}_{lt}"
                assert abs(loss.item() - float(g[key])) <= 2e-5 * abs(float(g[key])), key
                loss.backward()
                for which, s in (("src", a), ("dst", b)):
                    torch.testing.assert_close(prm[s][0].grad, T(g[key + f"_gR_{which}"]), rtol=2e-3, atol=2e-3)
                    torch.testing.assert_close(prm[s][1].grad, T(g[key + f"_gt_{which}"]), rtol=2e-3, atol=2e-3)


def _rgbd_case(tag):
    c = gc.RGBD
    inp = gc.rgbd_inputs()
    g = _load("samples")
    sel = list(range(c["n_frames"])) if tag == "all" else c["selected"]
    nf = len(sel)
    pb = torch.arange(nf).repeat_interleave(c["n_rays"])
    args = dict(depth=T(inp["depth"])[sel], T_WC=T(inp["T_WC"])[sel], R_wk=T(inp["R"])[sel], t_wk=T(inp["t"])[sel],
                intrinsics=(c["fx"], c["fy"], c["cx"], c["cy"]), pix_b=pb, pix_h=T(g[f"rgbd_{tag}_pix_h"]),
                pix_w=T(g[f"rgbd_{tag}_pix_w"]), u=T(g[f"rgbd_{tag}_u"]), g=T(g[f"rgbd_{tag}_g"]),
                normals=T(inp["normals"])[sel], frame_ids=torch.tensor(sel))
    knobs = {k: c[k] for k in ("min_depth", "dist_behind_surf", "trunc_dist", "n_strat", "n_surf")}
    return args, knobs, g


@pytest.mark.parametrize("tag", ["all", "sel"])
def test_rgbd_samples_match_reference(tag):
    """oracle.rgbd_sdf_samples vs the reference's PosedSdfRgbd.getitem_sdf on the same frames and draws."""
    args, knobs, g = _rgbd_case(tag)
    inputs, gt, extra = R.rgbd_sdf_samples(**args, **knobs)
    assert extra["n_first"] == g[f"rgbd_{tag}_u"].shape[0]
    assert inputs["coords_frame"].shape == g[f"rgbd_{tag}_coords"].shape
    # the frame change cancels two ~3 m terms: a few ulp of 3 m
    torch.testing.assert_close(inputs["coords_frame"], T(g[f"rgbd_{tag}_coords"]), rtol=0, atol=2e-6)
    assert torch.equal(inputs["sample_frame_ids"], T(g[f"rgbd_{tag}_ids"]))
    assert torch.equal(inputs["weights"], T(g[f"rgbd_{tag}_weights"]))
    torch.testing.assert_close(gt["sdf"], T(g[f"rgbd_{tag}_sdf"]), rtol=0, atol=1e-7)
    assert torch.equal(gt["sdf_valid"], T(g[f"rgbd_{tag}_valid"]))
    assert torch.equal(gt["sdf_signs"], T(g[f"rgbd_{tag}_signs"]))


def test_lidar_samples_match_reference():
    """oracle.lidar_frame_samples vs PosedSdf3DLidar.sample_frames, then the per-frame choice of getitem_world."""
    c = gc.LIDAR
    g = _load("samples")
    knobs = {k: c[k] for k in ("near_surface_n", "near_surface_std", "free_space_n", "behind_surface_n",
                               "trunc_dist", "min_dist_ratio", "max_range")}
    batch = {k: [] for k in ("points_frame", "sdfs", "sdfs_valid", "signs", "weights", "ids")}
    for f, fr in enumerate(gc.lidar_inputs()):
        pts = T(fr["points_global"])[T(g[f"lidar_perm_{f}"])]
        out = R.lidar_frame_samples(pts, T(fr["R"]), T(fr["t"]), T(g[f"lidar_g_near_{f}"]), T(g[f"lidar_u_free_{f}"]),
                                    T(g[f"lidar_u_behind_{f}"]), **knobs)
        for k, v in out.items():
            ref = T(g[f"lidar_{k}_{f}"])
            if k in ("sdfs_valid", "signs"):
                assert torch.equal(v, ref), k
            else:
                torch.testing.assert_close(v, ref, rtol=0, atol=4e-6, msg=k)
        pick = T(g[f"lidar_choice_{f}"])
        for k in ("points_frame", "sdfs", "sdfs_valid", "signs", "weights"):
            batch[k].append(out[k][pick])
        batch["ids"].append(torch.full((pick.numel(), 1), f, dtype=torch.int64))
    cat = {k: torch.cat(v) for k, v in batch.items()}
    torch.testing.assert_close(cat["points_frame"], T(g["lidar_batch_coords"]), rtol=0, atol=4e-6)
    torch.testing.assert_close(cat["sdfs"], T(g["lidar_batch_sdf"]), rtol=0, atol=4e-6)
    assert torch.equal(cat["ids"], T(g["lidar_batch_ids"]))
    assert torch.equal(cat["sdfs_valid"], T(g["lidar_batch_valid"]))
    assert torch.equal(cat["signs"], T(g["lidar_batch_signs"]))
    torch.testing.assert_close(cat["weights"], T(g["lidar_batch_weights"]), rtol=0, atol=1e-6)


# --------------------------------------------------------------------------- #
# The second backward of the sampler: the restatement against an independent fp64 oracle built from ATen alone
# (oracle.grid_sample_bwd2_aten) and against the reference's naive sampler (tests/golden/grad2_naive.npz)
# --------------------------------------------------------------------------- #
MODES = [(pad, ac) for pad in ("zeros", "border") for ac in (False, True)]


def _max_rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


@pytest.mark.parametrize("pad,ac", MODES)
@pytest.mark.parametrize("cot", ["ggx", "ggf", "both"])
def test_gather_double_backward_equals_aten_differences(pad, ac, cot):
    """(a) gg_out, g_x and g_feature of the restatement equal the ATen-built oracle to 1e-9 on FD-safe points, in- and
    out-of-bounds."""
    g = torch.Generator().manual_seed(11)
    f = torch.randn(1, 3, 5, 6, 7, generator=g, dtype=torch.float64)
    x = torch.rand(600, 3, generator=g, dtype=torch.float64) * 2.8 - 1.4
    go = torch.randn(600, 3, generator=g, dtype=torch.float64)
    ggx = torch.randn(600, 3, generator=g, dtype=torch.float64) if cot != "ggf" else None
    ggf = torch.randn(f.shape, generator=g, dtype=torch.float64) if cot != "ggx" else None
    safe = R.fd_safe(x, (7, 6, 5), ac)
    assert safe.sum() > 500
    x, go = x[safe], go[safe]
    ggx = None if ggx is None else ggx[safe]
    a = R.grid_sample_bwd2_aten(f, x, go, ggx, ggf, pad, ac)
    b = R.trilinear_bwd2(f, x, go, ggx, ggf, ac, pad)
    assert a[3].all()
    for u, v in zip(b, a[:3]):
        if v.abs().max() > 0:
            assert _max_rel(u, v) < 1e-9
        else:
            assert u.abs().max() == 0


def test_restatement_reproduces_the_reference_naive_sampler():
    """(b) tests/golden/grad2_naive.npz: the reference's naive_gridsample.py (border, align_corners=True) run as
    test3d.py:cmp_with_naive does, fp64.  Off the faces every output agrees; at a face the coordinate gradients follow
    ATen (set-grad zero at the clip limits), which naive does not at the lower face -- there the first coordinate
    gradient is checked against ATen instead."""
    g = _load("grad2_naive")
    n_face = 0
    for k in range(int(g["n_cases"])):
        image, optical = T(g[f"{k}_image"]), T(g[f"{k}_optical"])
        face = T(g[f"{k}_on_face"])
        n_face += int(face.sum())
        q = optical.reshape(-1, 3)

        def run(qq):
            im = image.clone().requires_grad_(True)
            qq = qq.clone().requires_grad_(True)
            out = R.trilinear_gather(im, qq, True, "border")
            gi, gq = torch.autograd.grad((out ** 2).sum(), [im, qq], create_graph=True)
            g2i, g2q = torch.autograd.grad(gi.sum() + gq.sum(), [im, qq])
            return out.detach(), gi.detach(), gq.detach(), g2i, g2q

        val, gi, gq, g2i, g2q = run(q)
        tol = dict(rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(val, T(g[f"{k}_value"]).reshape(val.shape[1], -1).t(), **tol)
        torch.testing.assert_close(gi, T(g[f"{k}_g_image"]), **tol)
        off = ~face
        torch.testing.assert_close(gq[off], T(g[f"{k}_g_optical"]).reshape(-1, 3)[off], **tol)
        torch.testing.assert_close(g2q[off], T(g[f"{k}_g2_optical"]).reshape(-1, 3)[off], **tol)
        if off.any():
            torch.testing.assert_close(run(q[off])[3], T(g[f"{k}_g2_image_off"]), **tol)
        if face.any():
            qa = q[face].clone().requires_grad_(True)
            b = R.grid_sample_stock(image, qa, True, "border")
            (ga,) = torch.autograd.grad((b ** 2).sum(), [qa])
            torch.testing.assert_close(gq[face], ga, **tol)
    assert n_face >= 20, "the lattice case must put points on the faces"


def _lattice_points(sizes_xyz, ac, n, g):
    """Normalised points whose unnormalised coordinates are half-integers from -1 to size (cell planes, edges,
    vertices, both faces, half a cell outside): dyadic for these sizes, hence exact in every step."""
    cols = []
    for s in sizes_xyz:
        i = torch.randint(-2, 2 * s + 1, (n,), generator=g).double() / 2
        cols.append(i * 2 / (s - 1) - 1 if ac else (2 * i + 1) / s - 1)
    return torch.stack(cols, 1)


@pytest.mark.parametrize("pad,ac", MODES)
def test_gather_first_derivatives_match_aten_on_planes_faces_and_vertices(pad, ac):
    """(c) value and first derivatives on the lattice itself, which random points never reach."""
    g = torch.Generator().manual_seed(3)
    sizes = (9, 5, 3) if ac else (8, 4, 2)
    inp = torch.randn(1, 2, sizes[2], sizes[1], sizes[0], generator=g, dtype=torch.float64)
    xn = _lattice_points(sizes, ac, 400, g)
    assert (~R.fd_safe(xn, sizes, ac)).float().mean() > 0.7     # on a plane in at least one axis
    go = torch.randn(400, 2, generator=g, dtype=torch.float64)
    outs = []
    for fn in (R.trilinear_gather, R.grid_sample_stock):
        i_, x_ = inp.clone().requires_grad_(True), xn.clone().requires_grad_(True)
        o = fn(i_, x_, ac, pad)
        outs.append((o.detach(), *torch.autograd.grad((o * go).sum(), [i_, x_])))
    for a, b in zip(*outs):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)


def test_encode_form_double_backward_two_ways():
    """(d) the encode form (bounds in metres as cfg-3, several levels, an ignored level): restatement = ATen-built oracle
    on FD-safe points, for ggx only, ggf on every level, ggf on one level."""
    g = torch.Generator().manual_seed(7)
    bound = torch.tensor([[-10.0, 10.0], [-5.0, 5.0], [-10.0, 10.0]], dtype=torch.float64)
    feats = [torch.randn(1, 2, z, y, x, generator=g, dtype=torch.float64) for (x, y, z) in ((6, 4, 5), (11, 7, 9), (20, 10, 20))]
    n = 500
    x = (torch.rand(n, 3, generator=g, dtype=torch.float64) * 1.2 - 0.1) * (bound[:, 1] - bound[:, 0]) + bound[:, 0]
    gout = torch.randn(n, 6, generator=g, dtype=torch.float64)
    ggx = torch.randn(n, 3, generator=g, dtype=torch.float64)
    ggf = [torch.randn(f.shape, generator=g, dtype=torch.float64) for f in feats]
    ign = [False, True, False]
    for e, gg in ((ggx, None), (ggx, ggf), (None, [ggf[0], None, None])):
        a = R.encode_bwd2_aten(feats, bound, x, gout, e, gg, ign)
        s = a[3]
        assert s.sum() > 400
        a = R.encode_bwd2_aten(feats, bound, x[s], gout[s], None if e is None else e[s], gg, ign)
        b = R.encode_bwd2_gather(feats, bound, x[s], gout[s], None if e is None else e[s], gg, ign)
        assert (a[0][:, 2:4] == 0).all() and (b[0][:, 2:4] == 0).all() and (a[2][1] == 0).all()
        for u, v in zip([b[0], b[1]] + b[2], [a[0], a[1]] + a[2]):
            if v.abs().max() > 0:
                assert _max_rel(u, v) < 1e-9
            else:
                assert u.abs().max() == 0
