"""The fp64 oracle of the tracker's device steps (oracle.ref_torch: track_pose64 .. adam6_64) and the bars
tests/test_tracker_steps_oracle.py judges the kernels with (tests/tracker_cases.py), on the CPU:

1. the staged oracle agrees with an independent route (R.lm_normal_equations + torch.linalg.solve; fp64 autograd through
   so3_exp_map -> transform_points_to -> sdf_gather -> MisoLossTracking's arithmetic) to 1e-9 of the yardsticks;
2. the cases are what they claim: a steep field, 50-90 % of rows kept and in bound, >= 90 % safe rows, a row swap in the
   near-origin solve, cond_inf within the solve bar's premise;
3. every bar accepts the oracle's own fp32 evaluation in the kernel's order and rejects each listed fault."""
import pytest
import torch

import tracker_cases as tc
from oracle import ref_torch as R

F32, F64 = torch.float32, torch.float64
ZERO3 = torch.zeros(3)


def _stage(kind, n, seed=0, dr2=0.0):
    """what the LM kernels see for one case, from the oracle alone: fp32 pose, mapped samples, fp64 field at them"""
    geo = tc.geometry(kind, n, seed)
    dr, dt = tc.correction(dr2, seed)
    pose = R.track_pose64(geo["R_base"], geo["t_base"], dr, dt).float()
    xw, x = R.track_transform32(geo["x"], pose)
    sdf, grad, premin = tc.field_eval(xw)
    keep = R.track_keep32(geo["target"], geo["trunc"])
    return dict(geo=geo, dr=dr, dt=dt, pose=pose, xw=xw, x=x, sdf=sdf, grad=grad, keep=keep,
                safe=tc.safe_rows(xw, premin), gt=geo["target"])


# --------------------------------------------------------------------------- the cases are what they claim
def test_the_field_is_steep_and_most_rows_are_kept_in_bound_and_safe():
    for n in (257, 33025):
        s = _stage("steep", n)
        med = s["grad"][s["safe"]].norm(dim=1).median().item()
        assert 0.2 <= med <= 2.0, med
        kept, inb, _, _ = R.track_counts(s["xw"], s["gt"], None, None, tc.KF, tc.TRUNC, tc.field()["bound"])
        assert 0.5 <= kept / n <= 0.9 and 0.5 <= inb / kept <= 0.9, (kept / n, inb / kept)
        assert s["safe"].float().mean().item() >= 0.9
        # J^T J / n against the damping: H dominates lambda from n = 64 on
        sums, _ = R.lm_sums64(s["x"], s["pose"], s["grad"], s["sdf"], s["gt"], s["keep"], "L2")
        H, _ = R.lm_unpack(sums)
        assert (H.diag() / kept).min().item() * 64 >= 2 * tc.LAMBDA["steep"]


@pytest.mark.parametrize("kind,n,seed", [("steep", n, s) for n, s in tc.LM_SEEDS["steep"].items()]
                         + [("near_origin", n, s) for n, s in tc.LM_SEEDS["near_origin"].items()])
def test_case_conditions_from_the_oracle(kind, n, seed):
    """at least one row kept; the near-origin system swaps rows (fp64 lu_factor pivots); cond_inf <= 1e4 for every steep
    case and the one-row near-origin case under L2.  The other near-origin cases measure cond_inf 1.8e4 .. 1.4e5 whatever
    the seed (the samples share one cell, so grad is nearly constant and both blocks of H are nearly rank one; one row under
    GM has w |J|^2 / lambda ~ 2e4): they are bounded by 1e6 here and judged by the backward-stability bound instead
    (tracker_cases.solve_bar)."""
    for lt in ("L2", "GM"):
        s = _stage(kind, n, seed)
        assert int(s["keep"].sum()) >= 1
        sums, _ = R.lm_sums64(s["x"], s["pose"], s["grad"], s["sdf"], s["gt"], s["keep"], lt, tc.GM_SCALE)
        lam = s["geo"]["lm_lambda"]
        _, cond = R.lm_solve64(sums.float(), lam)
        H, _ = R.lm_unpack(sums.float())
        _, piv = torch.linalg.lu_factor(H + lam * torch.eye(6, dtype=F64))
        swaps = int((piv != torch.arange(1, 7, dtype=piv.dtype)).sum())
        if kind == "near_origin":
            assert swaps >= 1 and piv[0] != 1, piv.tolist()
            assert cond <= (tc.COND_MAX if (n == 1 and lt == "L2") else 1e6), cond
        else:
            assert cond <= tc.COND_MAX, cond


# --------------------------------------------------------------------------- 1. two independent routes
@pytest.mark.parametrize("lt", ["L2", "GM"])
@pytest.mark.parametrize("kind,n,dr2", [("steep", 257, 0.09), ("steep", 65, 2.25), ("near_origin", 64, 0.0)])
def test_lm_oracle_agrees_with_the_dense_normal_equations(kind, n, dr2, lt):
    s = _stage(kind, n, 0, dr2)
    rows = s["keep"] & s["safe"]
    sums, A = R.lm_sums64(s["x"], s["pose"], s["grad"], s["sdf"], s["gt"], rows, lt, tc.GM_SCALE)
    i = torch.nonzero(rows).flatten()
    Rm = s["pose"][:9].view(3, 3).double()
    g32 = s["grad"].float().double()                       # lm_sums64 takes the kernel's fp32 values
    J, H, g = R.lm_normal_equations(s["x"].double()[i], Rm, g32[i], s["sdf"].float().double()[i, None],
                                    s["gt"].double()[i, None], lt, tc.GM_SCALE)
    Ho, go = R.lm_unpack(sums)
    Ha, ga = R.lm_unpack(A)
    assert ((Ho - H).abs() <= 1e-9 * Ha + 1e-300).all() and ((go - g[:, 0]).abs() <= 1e-9 * ga + 1e-300).all()
    assert sums[28] == i.numel()
    lam = s["geo"]["lm_lambda"]
    delta, cond = R.lm_solve64(sums, lam)
    want = torch.linalg.solve(H + lam * torch.eye(6, dtype=F64), -g)[:, 0]
    assert (delta - want).abs().max() <= 1e-9 * cond * want.abs().max()


@pytest.mark.parametrize("lt", ["L1", "L2", "GM"])
@pytest.mark.parametrize("dr2", [0.0, 2.5e-5, 4e-4, 0.09, 2.25])
def test_adam_oracle_agrees_with_autograd_through_the_pose(dr2, lt):
    n, weight = 257, 1.7
    geo = tc.geometry("steep", n, 0)
    dr, dt = tc.correction(dr2, 3)
    lab = tc.labels("block_bool", geo, holes=True)
    ok = lab["valid"][:, 0] & R.track_keep32(lab["target"], tc.TRUNC)
    x, gt = geo["x"].double(), lab["target"][:, 0].double()
    fl = tc.field()
    # route A: autograd through the whole chain
    drv, dtv = dr.double().requires_grad_(True), dt.double().requires_grad_(True)
    Rm = geo["R_base"].double() @ R.so3_exp_map(drv.view(1, 3))[0]
    xw = R.transform_points_to(x, Rm, (geo["t_base"].double() + dtv).view(3, 1))
    _, _, premin = tc.field_eval(xw.detach())
    ok = ok & tc.safe_rows(xw.detach(), premin)
    pred = R.sdf_gather([f.double() for f in fl["feats"]], fl["bound"].double(), xw, [w.double() for w in fl["ws"]],
                        [b.double() for b in fl["bs"]])[:, 0]
    resid = torch.where(ok, pred - gt, torch.zeros_like(pred))
    if lt == "L2":
        val = torch.mean(resid ** 2)
    elif lt == "L1":
        val = torch.mean(torch.abs(resid))
    else:
        e = resid.detach()
        val = torch.mean(tc.GM_SCALE / (tc.GM_SCALE + e ** 2) ** 2 * resid ** 2)
    loss = weight * val
    gdr, gdt = torch.autograd.grad(loss, [drv, dtv])
    # route B: the staged oracle
    sdf, grad, _ = tc.field_eval(xw.detach())
    loss_o, gpred = R.track_loss64(sdf, gt, ok, n, lt, weight, tc.GM_SCALE)
    gx = gpred[:, None] * grad
    ps = torch.cat([(gx[:, :, None] * x[:, None, :]).sum(0).reshape(9), gx.sum(0)])      # fp64 inputs: no fp32 cast
    g6, a6 = R.track_pull_back64(geo["R_base"], dr, ps)
    assert abs(float(loss_o) - loss.item()) <= 1e-9 * abs(loss.item())
    assert ((g6 - torch.cat([gdr, gdt])).abs() <= 1e-9 * a6 + 1e-300).all(), (g6, gdr, gdt)
    assert int(ok.sum()) > n // 3 and g6.abs().max() > 0
    # and the sums of fp32 inputs, as the kernel's are, against the same contraction
    gx32 = gx.float()
    s32, A32 = R.track_pose_sums64(gx32, geo["x"])
    want = torch.cat([(gx32.double()[:, :, None] * x[:, None, :]).sum(0).reshape(9), gx32.double().sum(0)])
    assert ((s32 - want).abs() <= 1e-9 * A32).all()
    # the explicit restatement of the kernel's backward formula is the autograd Jacobian (the kernel forms |w|^2 in fp32:
    # theta is off by 2^-24 relative, so 1e-7 here, not 1e-9)
    assert ((tc.pull_back_formula(geo["R_base"], dr, ps) - g6).abs() <= 1e-7 * a6 + 1e-300).all()


def test_adam6_64_is_torch_adam():
    p = torch.tensor([0.3, -0.2, 0.1, 0.5, 0.0, -1.0], dtype=F64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=2e-3)
    q, m, v = p.detach().clone(), torch.zeros(6, dtype=F64), torch.zeros(6, dtype=F64)
    for t in range(1, 5):
        g = torch.sin(torch.arange(6, dtype=F64) * t + 1.0)
        p.grad = g.clone()
        opt.step()
        q, m, v = R.adam6_64(q, g, m, v, t, 2e-3)
        assert (q - p.detach()).abs().max() <= 1e-15


# --------------------------------------------------------------------------- 3. sensitivity of the bars
def _rejected(ex):
    return bool((ex > 0).any())


@pytest.mark.parametrize("lt", ["L2", "GM"])
@pytest.mark.parametrize("n", [257, 33025])
def test_normal_equation_bar_accepts_fp32_and_rejects_faults(n, lt):
    """1e-5 A + 1e-12 on the 29 sums: the fp32 evaluation reduced as the kernel reduces stays under a quarter of it; a
    dropped row, an included filtered row, R_base for the pose at |dr|^2 = 4e-4 and the unsquared Geman-McClure weight
    each leave it."""
    s = _stage("steep", n, 0, 4e-4)
    args = (s["x"], s["pose"], s["grad"], s["sdf"], s["gt"])
    sums, A = R.lm_sums64(*args, s["keep"], lt, tc.GM_SCALE)
    s32, _ = R.lm_sums64(*args, s["keep"], lt, tc.GM_SCALE, dtype=F32)
    ratio = ((s32 - sums).abs() / (tc.SUMS_REL * A + 1e-12)).max().item()
    print(f"fp32 evaluation of the normal equations, n={n} {lt}: worst |fp32 - fp64| / bar = {ratio:.3f}")
    assert ratio <= 0.25 and s32[28] == sums[28]
    assert not _rejected(tc.sums_excess(s32, sums, A, exact=(28,)))
    kept, out = torch.nonzero(s["keep"]).flatten(), torch.nonzero(~s["keep"]).flatten()
    # the row whose contribution to H is the median one: a typical row, not the largest
    for which, rows in (("dropped", kept), ("included", out)):
        k2 = s["keep"].clone()
        i = rows[len(rows) // 2]
        k2[i] = which == "included"
        bad, _ = R.lm_sums64(*args, k2, lt, tc.GM_SCALE)
        assert _rejected(tc.sums_excess(bad, sums, A, exact=(28,))[:28]), which     # beyond the count itself
    base = R.track_pose64(s["geo"]["R_base"], s["geo"]["t_base"], ZERO3, s["dt"]).float()
    bad, _ = R.lm_sums64(s["x"], base, s["grad"], s["sdf"], s["gt"], s["keep"], lt, tc.GM_SCALE)
    assert _rejected(tc.sums_excess(bad, sums, A, exact=(28,)))
    if lt == "GM":
        r = s["sdf"].float().double() - s["gt"].double()
        sw = (tc.GM_SCALE / (tc.GM_SCALE + r * r)).sqrt()
        bad, _ = R.lm_sums64(s["x"], s["pose"], s["grad"] * sw[:, None], s["sdf"].float().double() * sw, s["gt"].double() * sw,
                             s["keep"], "L2")
        assert _rejected(tc.sums_excess(bad, sums, A, exact=(28,)))


@pytest.mark.parametrize("kind,n,seed", [("steep", n, s) for n, s in tc.LM_SEEDS["steep"].items()]
                         + [("near_origin", n, s) for n, s in tc.LM_SEEDS["near_origin"].items()])
def test_solve_bar_accepts_the_kernels_algorithm_and_rejects_a_wrong_unpacking(kind, n, seed):
    """8 x the error of fp32 torch.linalg.solve (tracker_cases.solve_bar): lm_solve_kernel restated in fp32 passes; H[0][3]
    read from the wrong triangle slot does not.  In the near-origin cases the exchange of two rows that forgets the
    right-hand side is rejected.  Leaving the exchange out altogether is NOT a fault the bar can see: elimination without
    pivoting is a valid solve of this symmetric positive definite system (measured 0.0001 .. 1.2 x the bar, the same as with
    it) -- the figure is printed, not asserted."""
    for lt in ("L2", "GM"):
        s = _stage(kind, n, seed)
        sums = R.lm_sums64(s["x"], s["pose"], s["grad"], s["sdf"], s["gt"], s["keep"], lt, tc.GM_SCALE)[0].float().double()
        lam = s["geo"]["lm_lambda"]
        delta, cond, bar = tc.solve_bar(sums, lam)
        err = lambda **kw: (tc.solve32(sums, lam, **kw) - delta).abs().max().item() / bar
        print(f"{kind} n={n} {lt}: cond {cond:.3g}, bar/|delta| {bar / delta.abs().max().item():.2e}, kernel algorithm "
              f"{err():.3f}, wrong slot {err(wrong_slot=True):.3g}, no exchange {err(skip_swap=True):.3g}, exchange without "
              f"rhs {err(swap_without_rhs=True):.3g}")
        assert err() <= 1.0
        assert err(wrong_slot=True) > 1.0
        if kind == "near_origin":
            assert err(swap_without_rhs=True) > 1.0


@pytest.mark.parametrize("lt", ["L1", "L2", "GM"])
def test_loss_bars_accept_fp32_and_reject_faults(lt):
    n, weight = 33025, 1.7
    s = _stage("steep", n, 0, 0.09)
    lab = tc.labels("block_bool", s["geo"], holes=True)
    ok = lab["valid"][:, 0] & s["keep"]
    sdf32 = s["sdf"].float()
    loss, gpred = R.track_loss64(sdf32, s["gt"], ok, n, lt, weight, tc.GM_SCALE)
    within = lambda got: bool(((got - gpred).abs() <= tc.GPRED_REL * gpred.abs()).all())
    l32, g32 = tc.gpred32(sdf32, s["gt"], ok, n, lt, weight)
    worst = ((g32 - gpred).abs() / gpred.abs().clamp_min(1e-300))[ok].max().item() / tc.GPRED_REL
    print(f"fp32 evaluation of gpred, {lt}: worst relative error / bar = {worst:.3f}; loss {abs(l32 - float(loss)) / float(loss):.2e}")
    assert within(g32) and abs(l32 - float(loss)) <= tc.LOSS_REL * float(loss)
    assert (g32[~ok] == 0).all() and (gpred[~ok] == 0).all()
    bl, bg = tc.gpred32(sdf32, s["gt"], ok, n, lt, weight, mean_over_kept=True)
    assert not within(bg) and abs(bl - float(loss)) > tc.LOSS_REL * float(loss)
    if lt == "GM":
        bl, bg = tc.gpred32(sdf32, s["gt"], ok, n, lt, weight, gm_unsquared=True)
        assert not within(bg) and abs(bl - float(loss)) > tc.LOSS_REL * float(loss)


@pytest.mark.parametrize("dr2", tc.DR2)
def test_pull_back_and_adam_bars_accept_the_kernels_arithmetic_and_reject_faults(dr2):
    n, lr = 257, 2e-3
    s = _stage("steep", n, 0, dr2)
    ok = s["keep"]
    _, gpred = R.track_loss64(s["sdf"].float(), s["gt"], ok, n, "L2", 1.0)
    gx = (gpred[:, None] * s["grad"]).float()
    ps, A = R.track_pose_sums64(gx, s["x"])
    p32, _ = R.track_pose_sums64(gx, s["x"], F32)
    assert not _rejected(tc.sums_excess(p32, ps, A))
    ps = p32.float().double()                                                        # what the Adam kernel reads
    g6, a6 = R.track_pull_back64(s["geo"]["R_base"], s["dr"], ps)
    ok6 = lambda got: bool(((got - g6).abs() <= tc.PULL_REL * a6).all())
    assert ok6(tc.pull_back_formula(s["geo"]["R_base"], s["dr"], ps).float().double())     # through the fp32 g6
    assert not ok6(tc.pull_back_formula(s["geo"]["R_base"], s["dr"], ps, no_transpose=True))
    if dr2 == 0.09:
        assert not ok6(tc.pull_back_formula(s["geo"]["R_base"], s["dr"], ps, drop_dadb=True))
    # two Adam steps: fp32 as adam_one forms them against fp64; the bias correction of the step before is rejected
    prm = torch.cat([s["dr"], s["dt"]]).double()
    m = v = torch.zeros(6, dtype=F64)
    for t in (1, 2):
        want = R.adam6_64(prm, g6.float(), m, v, t, lr)
        got = tc.adam32(prm, g6.float(), m, v, t, lr)
        assert (got[0] - want[0]).abs().max() <= tc.param_atol(lr)
        for a, b in zip(got[1:], want[1:]):
            assert ((a - b).abs() <= tc.MOMENT_RTOL * b.abs() + 1e-300).all()
        if t == 2:
            bad = tc.adam32(prm, g6.float(), m, v, t - 1, lr)
            assert (bad[0] - want[0]).abs().max() > tc.param_atol(lr)
        prm, m, v = want


def test_pose_bar_accepts_fp32_and_rejects_the_base_rotation():
    """4 * 2^-23 on the pose: so3_exp_map and the product evaluated in fp32 pass at every |dr|^2; R_base alone does not
    from |dr|^2 = 4e-4 on"""
    geo = tc.geometry("steep", 64, 0)
    for dr2 in tc.DR2:
        dr, dt = tc.correction(dr2, 1)
        want = R.track_pose64(geo["R_base"], geo["t_base"], dr, dt)
        got = torch.cat([(geo["R_base"] @ R.so3_exp_map(dr.view(1, 3))[0]).reshape(9), geo["t_base"] + dt]).double()
        assert tc.pose_ratio(got, want) <= 1, (dr2, tc.pose_ratio(got, want))
        if dr2 >= 4e-4:
            base = torch.cat([geo["R_base"].reshape(9), geo["t_base"] + dt]).double()
            assert tc.pose_ratio(base, want) > 1


def test_transform32_and_counts_on_exact_faces():
    """the bit-exact map on dyadic inputs is the exact map, and the in-bound count includes the faces"""
    n = 65
    q = tc.face_rows(n)
    t = torch.tensor([0.25, -0.125, 1.0], dtype=F64)
    pose = torch.cat([torch.eye(3).reshape(9), t.float()])
    xw, _ = R.track_transform32((q - t).float(), pose)
    assert torch.equal(xw.double(), q)
    b = torch.tensor(tc.FACE_BOUND, dtype=F64)
    inside = ((q >= b[:, 0]) & (q <= b[:, 1])).all(1)
    assert inside[:6].all() and not inside[6:12].any()
    kept, inb, wrong, bad = R.track_counts(xw, torch.zeros(n), None, None, tc.KF, tc.TRUNC, tc.FACE_BOUND)
    assert (kept, inb, wrong, bad) == (n, int(inside.sum()), 0, 0)
    # sanitising: NaN -> 0, +-inf -> +-FLT_MAX, and the fp32 compares of the filter
    x = torch.tensor([[float("nan"), 1.0, 2.0], [float("inf"), 0.0, float("-inf")]])
    _, clean = R.track_transform32(x, pose)
    assert torch.equal(clean, torch.nan_to_num(x)) and clean[0, 0] == 0 and clean[1, 0] == torch.finfo(F32).max
    assert R.track_keep32(torch.tensor([0.25, -0.2499999, float("nan")]), 0.25).tolist() == [False, True, False]
