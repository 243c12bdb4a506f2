"""The tracker's two device steps (lm.hip: miso_lm_track_step, miso_track_adam_step; ops.LmTrackStep, ops.TrackAdamWindow)
stage by stage against the fp64 oracle of oracle.ref_torch, on the steep field of tests/tracker_cases.py.  Every stage is
fed the kernel's own fp32 inputs to that stage (its pose, its mapped samples, its field values, its sums), so what is
left is rounding, and every bar is an absolute-value yardstick that tests/test_tracker_oracle.py shows, on the CPU, to
accept an fp32 evaluation and to reject a dropped row, a wrong triangle slot, the base rotation for the pose, a broken
row exchange, the unsquared Geman-McClure weight, R gR for R^T gR, the missing a' / b' terms, the bias correction of the
step before and the mean over kept rows.  The worst |kernel - fp64| / bar per stage is printed at the end (DESIGN.md
section 2 records it)."""
import functools

import pytest
import torch

import tracker_cases as tc
from oracle import ref_torch as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
LR, WEIGHT = 2e-3, 1.7
_WORST, _BARS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    if _WORST:
        print("\nworst |kernel - fp64| / bar per stage:", {k: f"{v:.3f}" for k, v in _WORST.items()})
        print("measured bars:", {k: f"{v:.3e}" for k, v in _BARS.items()})


def _ratio(stage, value):
    value = float(value)
    _WORST[stage] = max(_WORST.get(stage, 0.0), value if value == value else float("inf"))
    return value


def _same_bits(a, b):
    """equal as fp32 bit patterns, any NaN equal to any NaN (the host and the device pick different quiet NaNs)"""
    a, b = a.detach().cpu().reshape(-1), b.detach().cpu().reshape(-1)
    both_nan = torch.isnan(a) & torch.isnan(b)
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | both_nan).all())


@functools.lru_cache(maxsize=None)
def _device_field(bound=None):
    from miso_amd import ops
    fl = tc.field()
    feats = [f.to(DEV).contiguous(memory_format=torch.channels_last_3d) for f in fl["feats"]]
    b = fl["bound"] if bound is None else torch.tensor(bound, dtype=F32)
    pack = ops.DecoderPack([w.to(DEV) for w in fl["ws"]], [v.to(DEV) for v in fl["bs"]])
    return feats, ops.GridMeta.from_bound(b), pack


@functools.lru_cache(maxsize=None)
def _grad_bar():
    """4 x the worst error of the oracle's own fp32 evaluation of the field gradient (sdf_gather in float32 + autograd)
    against fp64, over the safe rows of the 33 025-row steep case: one fp32 realisation is a sample, not a bound.  Every
    case draws from the same field, so the one measurement serves them all (a case of 1 or 63 rows has no worst error of
    its own to speak of)."""
    geo = tc.geometry("steep", 33025, 0)
    xw, _ = R.track_transform32(geo["x"], R.track_pose64(geo["R_base"], geo["t_base"], torch.zeros(3), torch.zeros(3)).float())
    _, g64, premin = tc.field_eval(xw)
    _, g32, _ = tc.field_eval(xw, F32)
    safe = tc.safe_rows(xw, premin)
    _BARS["field gradient, absolute (4 x the fp32 oracle's worst error)"] = bar = 4.0 * (g32.double() - g64)[safe].abs().max().item()
    return bar


def _to_device(lab, wrong_frames=0):
    """the label columns on the device with the layout's strides: (target, valid, frame_ids)"""
    if "block" not in lab:
        return lab["target"].to(DEV), None, None
    block = lab["block"].to(DEV)
    valid = (block[:, 1:2] > 0) if lab["valid"].dtype == torch.bool else block[:, 1:2]
    fid = lab["frame_ids"].clone()
    fid[:wrong_frames] = tc.KF + 1
    return block[:, 0:1], valid, fid.to(DEV)


def _corrections(dr, dt):
    """(S,3) correction tensors of three keyframes; the tracked one is row 1, handed over as a view"""
    g = torch.Generator().manual_seed(9)
    cr, ct = torch.randn(3, 3, generator=g) * 0.1, torch.randn(3, 3, generator=g) * 0.1
    cr[1], ct[1] = dr, dt
    return cr.to(DEV), ct.to(DEV)


def _host_labels(lab, step, n):
    """(x, gt, ok) as the kernels after the head read them: the sanitised copies, or the batch itself"""
    if lab["sanitize"]:
        c = step.clean.cpu()
        assert _same_bits(c[:3 * n], torch.nan_to_num(lab["x"])), "sanitised coordinates"
        assert _same_bits(c[3 * n:4 * n], torch.nan_to_num(lab["target"].reshape(-1))), "sanitised targets"
        ok = torch.ones(n, dtype=torch.bool) if lab["valid"] is None else \
            (torch.nan_to_num(lab["valid"].reshape(-1).float()) == 1.0)
        assert torch.equal(c[4 * n:5 * n], ok.float()), "validity column"
        return c[:3 * n].view(n, 3), c[3 * n:4 * n], ok
    ok = torch.ones(n, dtype=torch.bool) if lab["valid"] is None else \
        (lab["valid"].reshape(-1) if lab["valid"].dtype == torch.bool else lab["valid"].reshape(-1) == 1.0)
    return lab["x"], lab["target"].reshape(-1), ok


def _check_head(what, step, lab, geo, dr0, dt0, n):
    """pose against fp64; mapped samples and sanitised copies bit for bit"""
    pose = step.pose.cpu()
    want = R.track_pose64(geo["R_base"], geo["t_base"], dr0, dt0)
    assert _ratio("pose", tc.pose_ratio(pose, want)) <= 1, f"{what}: pose beyond 4 * 2^-23: {(pose.double() - want).abs().tolist()}"
    x, gt, ok = _host_labels(lab, step, n)
    xw = step.xw.cpu()
    emu, _ = R.track_transform32(lab["x"], pose, lab["sanitize"])
    assert _same_bits(xw, emu), f"{what}: mapped samples differ from the fp32 emulation at rows " \
        f"{torch.nonzero((xw != emu).any(1) & ~torch.isnan(xw).any(1)).flatten()[:8].tolist()}"
    return pose, x, gt, ok, xw


def _check_counters(what, step, info, xw, gt, ok, fid, trunc, bound):
    want = R.track_counts(xw, gt, ok, fid, tc.KF, trunc, bound)           # kept, in bound, wrong frame, invalid
    sums = step.sums.cpu()
    assert sums[32:36].tolist() == [float(v) for v in want], (what, sums[32:36].tolist(), want)
    assert [info[4], info[3], info[5], info[6]] == [float(v) for v in want], (what, info, want)
    assert step.info.cpu()[3:7].tolist() == info[3:7] and info[7] == 0.0
    return want


# --------------------------------------------------------------------------- the LM step
def _lm_run(kind, n, lt, dr2, layout, holes=False, wrong_frames=0):
    from miso_amd import ops
    seed = tc.LM_SEEDS.get(kind, {}).get(n, 0)
    bound = tc.FACE_BOUND if kind == "faces" else tc.CASE["bound"]
    feats, meta, pack = _device_field(None if kind != "faces" else tuple(map(tuple, tc.FACE_BOUND)))
    geo = tc.geometry(kind, n, seed)
    lab = tc.labels(layout, geo, holes=holes)
    dr0, dt0 = tc.correction(dr2, seed)
    if kind == "faces":
        dt0 = torch.zeros(3)                                            # the map stays exact: rows stay on the faces
    target, valid, fid = _to_device(lab, wrong_frames)
    cr, ct = _corrections(dr0, dt0)
    cr0, ct0 = cr.clone(), ct.clone()
    step = ops.LmTrackStep(n, DEV, pack)
    lam = geo["lm_lambda"]
    info = step(feats, meta, pack, lab["x"].to(DEV), target, valid, fid, tc.KF, lab["trunc"], geo["R_base"].to(DEV),
                geo["t_base"].to(DEV), cr[1], ct[1], lt, tc.GM_SCALE, lam, sanitize=lab["sanitize"])
    what = f"{kind} n={n} {lt} |dr|^2={dr2} {layout}"
    pose, x, gt, ok, xw = _check_head(what, step, lab, geo, dr0, dt0, n)
    cnt = _check_counters(what, step, info, xw, gt, ok, None if fid is None else fid.cpu(), lab["trunc"], bound)
    for k in (0, 2):                                                    # the other keyframes
        assert torch.equal(cr[k], cr0[k]) and torch.equal(ct[k], ct0[k])
    return dict(what=what, step=step, info=info, geo=geo, lab=lab, pose=pose, x=x, gt=gt, ok=ok, xw=xw, cnt=cnt, lam=lam,
                before=(cr0[1].cpu(), ct0[1].cpu()), after=(cr[1].cpu(), ct[1].cpu()), kind=kind, lt=lt, n=n)


def _check_field(r):
    """the kernel's SDF and spatial gradient at its own mapped samples, on the rows where the field is smooth"""
    sdf64, g64, premin = tc.field_eval(r["xw"])
    safe = tc.safe_rows(r["xw"], premin)
    if not safe.any():
        return
    sdf, grad = r["step"].sdf.cpu().double(), r["step"].grad.cpu().double()
    bar = tc.SDF_REL * max(1.0, sdf64[safe].abs().max().item())
    e = (sdf - sdf64)[safe].abs().max().item()
    _ratio("field sdf", e / bar)
    assert e <= bar, f"{r['what']}: sdf off by {e:.3e} (bar {bar:.3e})"
    eg = (grad - g64)[safe].abs().max().item()
    _ratio("field gradient", eg / _grad_bar())
    assert eg <= _grad_bar(), f"{r['what']}: d sdf / dx off by {eg:.3e} (bar {_grad_bar():.3e})"


def _check_normal_equations(r):
    step = r["step"]
    keep = R.track_keep32(r["gt"], r["lab"]["trunc"])
    sums, A = R.lm_sums64(r["x"], r["pose"], step.grad.cpu(), step.sdf.cpu(), r["gt"], keep, r["lt"], tc.GM_SCALE)
    got = step.sums.cpu()[:29].double()
    ex = tc.sums_excess(got, sums, A, exact=(28,))
    pos = A > 0
    if pos.any():
        _ratio("normal equations", ((got - sums).abs()[pos] / (tc.SUMS_REL * A[pos] + 1e-12)).max())
    bad = torch.nonzero(ex > 0).flatten().tolist()
    assert not bad, f"{r['what']}: sums {bad} beyond 1e-5 A: |d| {(got - sums).abs()[bad].tolist()} A {A[bad].tolist()}"
    return got


def _check_solve(r, got):
    delta, cond, bar = tc.solve_bar(got, r["lam"])
    assert cond <= (tc.COND_MAX if r["kind"] != "near_origin" else 1e6), (r["what"], cond)
    if cond <= tc.COND_MAX:
        key = "solve, largest bar / |delta|_inf at cond <= 1e4 (8 x fp32 torch.linalg.solve)"
        _BARS[key] = max(_BARS.get(key, 0.0), bar / max(delta.abs().max().item(), 1e-300))
    b, a = torch.cat(r["before"]).double(), torch.cat(r["after"]).double()
    err = ((a - b) - delta).abs() - tc.EPS32 * a.abs()                  # the in-place add rounds to the correction's ulp
    _ratio("solve" if cond <= tc.COND_MAX else "solve (cond > 1e4: backward bound)", err.max().item() / bar + 0.0)
    assert err.max().item() <= bar, f"{r['what']}: update {(a - b).tolist()} against {delta.tolist()}, cond {cond:.3g}, bar {bar:.3e}"
    _, g = R.lm_unpack(got)
    info = r["info"]
    for i, (have, want) in enumerate(((info[0], delta[:3].norm().item()), (info[1], delta[3:].norm().item()),
                                      (info[2], g.norm().item()))):
        assert abs(have - want) <= tc.NORM_REL * want + (2 * bar if i < 2 else 0.0), (r["what"], i, have, want)


# every size with every |dr|^2 on the steep geometry, the loss and the layout rotating so that each loss meets each layout;
# the near-origin geometry where its conditions were asserted (tests/test_tracker_oracle.py)
LM_CASES = [("steep", n, ("L2", "GM")[(i + j) % 2], dr2, tc.LAYOUTS[(i + j) % 5])
            for i, n in enumerate(tc.SIZES) for j, dr2 in enumerate(tc.DR2)] + \
    [("near_origin", 1, "L2", 0.0, "plain"), ("near_origin", 64, "L2", 0.0, "block_bool"),
     ("near_origin", 257, "GM", 0.0, "sanitize"), ("near_origin", 64, "GM", 0.0, "block_float")]


@pytest.mark.parametrize("kind,n,lt,dr2,layout", LM_CASES)
def test_lm_step_stage_by_stage(kind, n, lt, dr2, layout):
    r = _lm_run(kind, n, lt, dr2, layout)
    assert r["cnt"][2] == 0 and r["cnt"][3] == 0
    _check_field(r)
    got = _check_normal_equations(r)
    _check_solve(r, got)
    if kind == "near_origin":                                           # the case is about the row exchange
        H, _ = R.lm_unpack(got)
        _, piv = torch.linalg.lu_factor(H + r["lam"] * torch.eye(6, dtype=F64))
        assert piv[0] != 1, piv.tolist()


@pytest.mark.parametrize("n", [12, 65])
def test_lm_step_counts_rows_on_exact_faces(n):
    """identity rotation, dyadic translation and samples: the mapped samples are exact, six rows sit ON the faces of the
    bound (counted: the test is inclusive) and six one lattice step outside"""
    r = _lm_run("faces", n, "L2", 0.0, "plain")
    q = tc.face_rows(n)
    assert torch.equal(r["xw"].double(), q)
    b = torch.tensor(tc.FACE_BOUND, dtype=F64)
    inside = ((q >= b[:, 0]) & (q <= b[:, 1])).all(1)
    assert inside[:6].all() and not inside[6:12].any()
    assert r["cnt"][:2] == (n, int(inside.sum()))
    _check_solve(r, _check_normal_equations(r))


@pytest.mark.parametrize("why", ["wrong_frame", "invalid"])
def test_lm_step_leaves_the_pose_alone_when_the_reference_would_assert(why):
    """rows of another keyframe / invalid rows among the kept ones: the counters say so, info is written, and the
    corrections keep their bits"""
    r = _lm_run("steep", 257, "L2", 4e-4, "block_bool", holes=why == "invalid", wrong_frames=40 if why == "wrong_frame" else 0)
    assert r["cnt"][2 if why == "wrong_frame" else 3] > 0 and r["cnt"][3 if why == "wrong_frame" else 2] == 0
    assert _same_bits(r["after"][0], r["before"][0]) and _same_bits(r["after"][1], r["before"][1])
    got = _check_normal_equations(r)                                    # the step was still computed ...
    delta, _, bar = tc.solve_bar(got, r["lam"])
    assert abs(r["info"][0] - delta[:3].norm().item()) <= tc.NORM_REL * delta[:3].norm().item() + 2 * bar      # ... and reported


def test_lm_step_with_no_rows_at_the_c_level():
    """the Python tracker returns before the call when the batch is empty; the library itself answers 0 with a zero
    update and zero counters (H = lambda I)"""
    from miso_amd import ops
    feats, meta, pack = _device_field()
    dr0, dt0 = tc.correction(0.09, 0)
    cr, ct = _corrections(dr0, dt0)
    step = ops.LmTrackStep(0, DEV, pack)
    info = step(feats, meta, pack, torch.empty(0, 3, device=DEV), torch.empty(0, device=DEV), None, None, tc.KF, tc.TRUNC,
                torch.eye(3, device=DEV), torch.zeros(3, device=DEV), cr[1], ct[1], "L2", tc.GM_SCALE, 0.5)
    assert info == [0.0] * 8
    assert step.sums.cpu().tolist() == [0.0] * 36
    assert torch.equal(cr[1].cpu(), dr0) and torch.equal(ct[1].cpu(), dt0)


# --------------------------------------------------------------------------- the Adam window
def _adam_window(n, lt, dr2, layout, steps=4, table=4, feats=None, after_step=None):
    """run ``steps`` iterations in lockstep with the oracle; returns the window and the last iteration's record"""
    from miso_amd import ops
    dfeats, meta, pack = _device_field()
    feats = dfeats if feats is None else feats
    seed = tc.LM_SEEDS["steep"].get(n, 0)
    geo = tc.geometry("steep", n, seed)
    lab = tc.labels(layout, geo, holes=True)
    dr0, dt0 = tc.correction(dr2, seed)
    target, valid, fid = _to_device(lab)
    cr, ct = _corrections(dr0, dt0)
    cr0, ct0 = cr.clone(), ct.clone()
    win = ops.TrackAdamWindow(n, DEV, pack, LR, table)
    win.reset()
    xd, Rb, tb = lab["x"].to(DEV), geo["R_base"].to(DEV), geo["t_base"].to(DEV)
    what = f"adam n={n} {lt} |dr|^2={dr2} {layout}"
    nan_run = bool(torch.isnan(feats[0]).any())
    rec = None
    for it in range(steps):
        dr_b, dt_b, st_b = cr[1].cpu(), ct[1].cpu(), win.state.cpu()
        win.step(feats, meta, pack, xd, target, valid, fid, tc.KF, lab["trunc"], Rb, tb, cr[1], ct[1], lt, WEIGHT,
                 tc.GM_SCALE, sanitize=lab["sanitize"])
        torch.cuda.synchronize()
        w = f"{what} it={it}"
        pose, x, gt, ok, xw = _check_head(w, win, lab, geo, dr_b, dt_b, n)
        ok = ok & R.track_keep32(gt, lab["trunc"])
        st, cnt_b, cnt = win.state.cpu(), st_b[12:15].view(torch.int32).tolist(), win.state.cpu()[12:15].view(torch.int32).tolist()
        ring, info0 = win.ring.cpu(), win.info.cpu()[0].item()
        if nan_run:
            assert cnt == [cnt_b[0], cnt_b[1] + 1, cnt_b[2] + 1], (w, cnt_b, cnt)
            assert _same_bits(st[:12], st_b[:12]) and _same_bits(cr[1], dr_b) and _same_bits(ct[1], dt_b), w
            assert info0 != info0 and (it >= table or ring[it] != ring[it]), w
            continue
        # loss and d loss / d sdf from the kernel's own SDF
        sdf = win.sdf.cpu()
        loss, gpred = R.track_loss64(sdf, gt, ok, n, lt, WEIGHT, tc.GM_SCALE)
        gp = win.gpred.cpu().double()
        assert (gp[~ok] == 0).all(), f"{w}: filtered / invalid rows carry a gradient"
        live = ok & (gpred != 0)
        if live.any():
            _ratio("gpred", ((gp - gpred).abs()[live] / gpred.abs()[live]).max() / tc.GPRED_REL)
        assert ((gp - gpred).abs() <= tc.GPRED_REL * gpred.abs()).all(), \
            f"{w}: gpred rows {torch.nonzero((gp - gpred).abs() > tc.GPRED_REL * gpred.abs()).flatten()[:8].tolist()}"
        _ratio("loss", abs(info0 - float(loss)) / max(abs(float(loss)), 1e-300) / tc.LOSS_REL)
        assert abs(info0 - float(loss)) <= tc.LOSS_REL * abs(float(loss)), (w, info0, float(loss))
        if it < table:
            assert ring[it].item() == info0, w
        # pose cotangents from the kernel's own d loss / d x_world
        sums = win.sums.cpu().double()
        ps, A = R.track_pose_sums64(win.grad.cpu(), x)
        ex = tc.sums_excess(sums[:12], ps, A)
        if (A > 0).any():
            _ratio("pose sums", ((sums[:12] - ps).abs()[A > 0] / (tc.SUMS_REL * A[A > 0] + 1e-12)).max())
        assert not (ex > 0).any(), f"{w}: pose sums {torch.nonzero(ex > 0).flatten().tolist()} beyond 1e-5 A"
        assert sums[12].item() == info0
        # pull-back and Adam from the kernel's sums and the state before the step
        t = cnt_b[0] + 1
        g6, a6 = R.track_pull_back64(geo["R_base"], dr_b, sums[:12])
        want_p, want_m, want_v = R.adam6_64(torch.cat([dr_b, dt_b]), g6, st_b[:6], st_b[6:12], min(t, table), LR)
        if t == 1:
            g_in = st[:6].double() / (1.0 - 0.9)                        # m after the first step is (1 - beta1) g
            _ratio("pull-back", ((g_in - g6).abs() / (tc.PULL_REL * a6).clamp_min(1e-300)).max())
            assert ((g_in - g6).abs() <= tc.PULL_REL * a6).all(), (w, g_in.tolist(), g6.tolist(), a6.tolist())
        got_p = torch.cat([cr[1].cpu(), ct[1].cpu()]).double()
        _ratio("adam parameters", (got_p - want_p).abs().max() / tc.param_atol(LR))
        assert (got_p - want_p).abs().max() <= tc.param_atol(LR), (w, got_p.tolist(), want_p.tolist())
        for name, have, want in (("m", st[:6].double(), want_m), ("v", st[6:12].double(), want_v)):
            nz = want != 0
            if nz.any():
                _ratio("adam moments", ((have - want).abs()[nz] / want.abs()[nz]).max() / tc.MOMENT_RTOL)
            assert ((have - want).abs() <= tc.MOMENT_RTOL * want.abs() + 1e-30).all(), (w, name, have.tolist(), want.tolist())
        assert cnt == [t, cnt_b[1], cnt_b[2] + 1], (w, cnt_b, cnt)
        rec = dict(sdf=sdf, ok=ok, gp=gp, gt=gt, target=target, lab=lab)
        if after_step is not None:
            after_step(it, rec, cr, ct, dr_b, dt_b, win)
    for k in (0, 2):                                                    # the other keyframes' rows of the (S,3) tensors
        assert torch.equal(cr[k], cr0[k]) and torch.equal(ct[k], ct0[k])
    return win, rec, (cr, ct, cr0, ct0)


ADAM_CASES = [(n, ("L1", "L2", "GM")[(i + 2 * j) % 3], dr2, tc.LAYOUTS[(i + j) % 5])
              for i, n in enumerate(tc.SIZES) for j, dr2 in enumerate(tc.DR2)]


@pytest.mark.parametrize("n,lt,dr2,layout", ADAM_CASES)
def test_adam_window_stage_by_stage(n, lt, dr2, layout):
    win, rec, _ = _adam_window(n, lt, dr2, layout)
    losses, steps, skipped = win.finish()
    assert (len(losses), steps, skipped) == (4, 4, 0)
    assert rec is not None and (n == 1 or int(rec["ok"].sum()) > 0)


def test_adam_window_l1_at_a_residual_of_exactly_zero():
    """eight targets are replaced by the kernel's own SDF values and the pose is put back: those rows have r = 0 exactly,
    and their d loss / d sdf is +-0, not +-weight / n"""
    n = 257
    picked = []

    def after(it, rec, cr, ct, dr_b, dt_b, win):
        if it == 0:
            rows = torch.nonzero(rec["ok"] & (rec["sdf"].abs() < 0.9 * tc.TRUNC)).flatten()[:8]
            assert rows.numel() == 8 and (rec["gp"][rows] != 0).all()
            picked.append(rows)
            rec["target"][rows.to(DEV), 0] = rec["sdf"][rows].to(DEV)
            rec["lab"]["block"][rows, 0] = rec["sdf"][rows]              # the host copy the oracle reads (target views it)
            cr[1].copy_(dr_b.to(DEV))
            ct[1].copy_(dt_b.to(DEV))
        else:
            rows = picked[0]
            assert rec["ok"][rows].all() and torch.equal(rec["sdf"][rows], rec["gt"][rows])
            assert (rec["gp"][rows] == 0).all(), rec["gp"][rows].tolist()
            assert (rec["gp"][rec["ok"]] != 0).sum() == int(rec["ok"].sum()) - 8

    _adam_window(n, "L1", 4e-4, "block_bool", steps=2, after_step=after)


def test_adam_window_skips_a_nan_loss():
    """NaN features: the loss is NaN, nothing in dr, dt, m, v moves (bit for bit), skipped and iterations count up, and the
    ring entry is NaN"""
    feats, _, _ = _device_field()
    bad = [torch.full_like(feats[0], float("nan"))] + list(feats[1:])
    win, _, _ = _adam_window(257, "L2", 0.09, "block_bool", steps=3, feats=bad)
    losses, steps, skipped = win.finish()
    assert (steps, skipped, len(losses)) == (0, 3, 3) and all(l != l for l in losses)


def test_adam_window_past_the_end_of_its_scalar_table():
    """a window built for 2 iterations and run for 4: steps 3 and 4 use the table's last row (the bias corrections of
    step 2 -- _adam_window hands adam6_64 min(t, 2)), the loss ring keeps its 2 entries, and finish() reports 2 losses and 4
    steps"""
    win, _, _ = _adam_window(65, "L2", 0.09, "block_float", steps=4, table=2)
    assert win.ring.shape[0] == 2 and win.table.shape[0] == 2
    losses, steps, skipped = win.finish()
    assert (len(losses), steps, skipped) == (2, 4, 0)
    assert win.state[12:15].view(torch.int32).cpu().tolist() == [4, 0, 4]
