"""What tests/test_atlas_oracle.py (GPU) rests on, on the CPU: the fp64 oracle of the fused atlas query and its backward
(oracle.atlas64) against fp64 autograd of the reference's formula, every case of tests/atlas_cases.py against the
conditions it states, and the bars against an fp32 restatement of the package's loop and ten planted faults."""
import pytest
import torch

import atlas_cases as A
from oracle import ref_torch as R

F32, F64 = torch.float32, torch.float64
FORMS = ("exact_fp32", "split")


def literal64(a, x, gsdf, xl32):
    """fp64 autograd of the reference formula (grid_atlas.py:374-399): per submap transfrom_points_from -- as
    transform_points_to with the table's (R^T, -R^T t) --, coords_in_bound, encode_stock (F.grid_sample per level),
    the masked sum, the count clamp, the decoder.  The local coordinate and every level's normalised coordinate carry
    the VALUE of the kernel's fp32 one (its fp64 image) and the derivative of the formula's own chain: at 1e-12 of the
    yardsticks nothing else can be compared with an oracle that stands on the kernel's coordinates."""
    S = len(a.feats)
    x = x.double().clone().requires_grad_(True)
    poses = a.poses.double().clone().requires_grad_(True)
    feats = [[f.double().clone().requires_grad_(s not in a.locked) for f in fs] for s, fs in enumerate(a.feats)]
    total, count = 0, 0
    for s in range(S):
        moved = R.transform_points_to(x, poses[s, :9].view(3, 3), poses[s, 9:, None])
        bound = torch.tensor(a.bounds[s], dtype=F64)
        inside = R.coords_in_bound(xl32[s].double(), bound)
        rows = []
        for l, f in enumerate(feats[s]):
            size = torch.tensor([f.shape[4], f.shape[3], f.shape[2]], dtype=F64)
            ix, mult = R.sample_index32(xl32[s], a.bounds[s], (f.shape[4], f.shape[3], f.shape[2]))
            xn = ((2 * ix + 1) / size - 1) + (2 / size) * mult * (moved - moved.detach())
            v = R.grid_sample_stock(f, xn)
            if a.ignore is not None and a.ignore[s] is not None and a.ignore[s][l]:
                v = torch.zeros_like(v)
            rows.append(v)
        total = total + inside * torch.cat(rows, 1)
        count = count + inside
    count = count.double()
    count[count == 0] = 1
    mean = total / count
    sdf = R.mlp_forward(mean, [w.double() for w in a.ws], [b.double() for b in a.bs])
    (gsdf.double()[:, None] * sdf).sum().backward()
    grids = [[None if s in a.locked else (torch.zeros_like(f) if f.grad is None else f.grad) for f in fs]
             for s, fs in enumerate(feats)]
    return A.Outputs(mean.detach(), sdf.detach()[:, 0], x.grad, poses.grad, grids)


@pytest.mark.parametrize("name", A.SMALL_CASES)
def test_oracle_equals_float64_autograd_of_the_reference_formula(name):
    """on every finite row whose fp32 membership is the float64 one (the others are counted and shown: there the kernel
    follows fp32, and so does the oracle), to 1e-12 of the yardsticks"""
    c = A.case(name)
    a = c.atlas
    fin = torch.isfinite(c.x).all(1)
    agree = fin & (A.inside64(a, torch.nan_to_num(c.x)) == c.o.inside).all(1)
    print(f"{name}: {int(fin.sum() - agree.sum())} of {int(fin.sum())} finite rows are inside a submap in fp32 and outside "
          f"it in float64, or the reverse; {int((~fin).sum())} rows are not finite")
    x, g = c.x[agree], c.gsdf[agree]
    o = A.oracle(a, x, g)
    got = literal64(a, x, g, o.xl)
    # a vertex's gradient also gets an absolute term: grid_sample forms its index coordinate from xn again, to ~1e-14
    # of a cell, and a vertex that only rows next to a cell plane reach has a yardstick (sum |g| w) of that size
    slack = 1e-13 * o.dfeat.abs().max().item() if o.dfeat.numel() else 0.0
    pairs = [(got.feat, o.feat, 1e-12 * o.feat_y), (got.sdf, o.sdf, 1e-12 * o.sdf_y), (got.gx, o.gx, 1e-12 * o.gx_y),
             (got.gposes, o.gposes, 1e-12 * o.gposes_y)]
    pairs += [(g_, w, 1e-12 * y + slack) for gs, ws, ys in zip(got.grids, o.grids, o.grids_y) for g_, w, y in zip(gs, ws, ys)
              if w is not None]
    for i, (g_, w, tol) in enumerate(pairs):
        tol = tol + 1e-18
        assert g_.shape == w.shape and bool(((g_ - w).abs() <= tol).all()), \
            f"{name}: output {i}: {((g_ - w).abs() / tol).max().item():.2f} x the tolerance"
    for gs, ws in zip(got.grids, o.grids):
        assert [g_ is None for g_ in gs] == [w is None for w in ws]


def test_frame_change_is_the_exact_one_where_it_is_exact():
    """signed-permutation rotations and dyadic translations: every product is exact, so the restatement's local
    coordinate is the float64 one rounded ONCE (the sum x + t), and rows exist that this rounding puts onto a face
    the float64 coordinate lies beyond: the kernel has to follow fp32 there"""
    c = A.case("exact")
    a = c.atlas
    fin = torch.isfinite(c.x).all(1)
    x64 = c.x[fin].double()
    for s in range(len(a.feats)):
        Rw, t = a.world[s]
        assert torch.equal(c.o.xl[s][fin], R.transfrom_points_from(x64, Rw, t[:, None]).float())
    differ = (A.inside64(a, x64) != c.o.inside[fin]).any(1)
    faces = c.kind[fin] == A.K["faces"]
    assert int((differ & faces).sum()) >= 8 and not bool((differ & ~faces).any())


@pytest.mark.parametrize("name", A.SMALL_CASES + A.STRIDE_CASES)
def test_case_meets_its_conditions(name):
    c = A.case(name)
    a, o, n = c.atlas, c.o, c.x.shape[0]
    S = len(a.feats)
    assert (a.C, a.L, a.H) in {(8, 3, 64), (8, 4, 64), (4, 2, 32), (4, 1, 32)}
    assert all(max(f.shape[2:]) <= 32 for fs in a.feats for f in fs)
    # ties: a condition on the case, at most 1 row in 1000, and they carry no cotangent
    assert int(o.tie.sum()) * 1000 <= max(n, 1000), f"{name}: {int(o.tie.sum())} tie rows of {n}"
    assert not bool(c.gsdf[o.tie].any()) and torch.equal(o.gsdf.float(), c.gsdf)
    # non-finite rows are inside nothing and have exactly nothing
    bad = ~(c.x.abs() < 1e29).all(1)      # NaN, +-inf and 1e30
    assert not bool(o.inside[bad].any()) and not bool(o.feat[bad].any()) and not bool(o.gx[bad].any())
    assert bool((o.sdf[o.count == 0] == o.sdf_zero).all())
    assert all(bool(torch.isfinite(t).all()) for t in (o.feat, o.sdf, o.gx, o.gposes))
    if name in A.CASE_ATLAS:
        k = lambda kind: c.kind == A.K[kind]      # noqa: E731
        rows = torch.arange(n)
        assert bool((k("empty") == (rows < 64)).all()) and bool((k("lonely") == ((rows >= 64) & (rows < 192))).all())
        assert bool((k("alone") == ((rows >= 192) & (rows < 256))).all()) and bool((k("mixed") == ((rows >= 256) & (rows < 320))).all())
        assert not bool(o.inside[:64].any()), "the empty run is not empty"
        assert o.inside[64:128].any(1).nonzero().flatten().tolist() == [0], "lonely run, lane 0"
        assert o.inside[128:192].any(1).nonzero().flatten().tolist() == [63], "lonely run, lane 63"
        assert bool(bad[192:256].all()) and int(bad[256:320].sum()) == 12 and bool(o.inside[256:320].any())
        assert int((~torch.isfinite(c.x[256:320])).any(1).sum()) == 9
        assert int(k("faces").sum()) == S * 26 * 7
        both = o.inside[k("faces")]
        assert bool(both.any()) and not bool(both.any(1).all()), "face rows on one side only"
    if name in ("generic84", "generic42"):
        pops = [int(((o.count == k) & (c.kind == A.K["interior"])).sum()) for k in range(S + 1)]
        assert S == 5 and min(pops) >= 50, f"{name}: interior rows per count {pops}"
        assert float(a.poses[:, 9:].abs().max()) > 5.0      # (the frame change cancels)
    if name == "many":
        assert S == 48 and 12 * S > 512 and 12 * S > 256 and 12 * (S - 1) > 512
        assert all(bool(o.inside[:, s].any()) for s in range(S)) and bool((o.gposes[43:].abs() > 0).all())
    if name == "ignored":
        assert any(ig is not None and any(ig) for ig in a.ignore)
    if name == "locked":
        assert a.locked and all(g is None for s in a.locked for g in o.grids[s])
    if name in A.STRIDE_CASES:
        assert S == 2 and n == (A.N_STRIDE_BWD if name == "stride_bwd" else A.N_STRIDE_FWD)


MEASURED = {}      # case -> the restatement's worst ratio per output


@pytest.mark.parametrize("name", A.SMALL_CASES + A.STRIDE_CASES)
def test_bars_accept_the_fp32_restatement(name):
    c = A.case(name)
    got = A.loop32(c)
    for form in FORMS:
        A.check_outputs(form, f"loop32/{name}", got, c)
    r = MEASURED[name] = A.ratios(got, c)
    print(f"{name}: fp32 restatement, worst |fp32 - fp64| / (u yardstick):", {k: f"{v:.3f}" for k, v in r.items()})


def test_the_measured_constants_are_the_restatements():
    """k = 2 x (4 x: split) RESTATEMENT: no constant is below what the restatement measures here over all cases by more
    than a CPU's math library moves it (a quarter either way was seen between two machines on other fp32
    restatements of this suite; the bars themselves, at 2 x, accept it in test_bars_accept_the_fp32_restatement),
    and none is more than four times it"""
    for name in A.SMALL_CASES + A.STRIDE_CASES:
        if name not in MEASURED:      # (this test run alone)
            MEASURED[name] = A.ratios(A.loop32(A.case(name)), A.case(name))
    worst = {k: max(r[k] for r in MEASURED.values()) for k in ("sdf", "gx", "gposes", "grids")}
    print("worst ratios of the fp32 restatement over all cases:", {k: f"{v:.3f}" for k, v in worst.items()})
    for k, v in worst.items():
        assert 0.25 * A.RESTATEMENT[k] <= v <= 1.25 * A.RESTATEMENT[k], (k, v, A.RESTATEMENT[k])
    assert A.kbar("exact_fp32", "gposes", 1000) == 2 * A.RESTATEMENT["gx"] + 16
    assert A.kbar("exact_fp32", "gposes", A.N_STRIDE_BWD) == 2 * A.RESTATEMENT["gx"] + 24


def test_grid_atlas_case_and_the_corrections_bar():
    """GridAtlas on the CPU: the case the GPU module builds on the device, its restatement within every bar, and the
    pose-table gradient pulled back to the corrections through the fp32 chain within the corrections' bar"""
    m = A.module_atlas("cpu")
    with torch.no_grad():
        table = m._pose_table("cpu")
    c = A.module_case(m, table)
    assert (c.atlas.C, c.atlas.L, c.atlas.H) == (4, 2, 32) and int(c.o.tie.sum()) * 1000 <= c.x.shape[0]
    assert all(float(m.rotation_corrections[s].abs().max()) > 1e-3 for s in range(5))
    got = A.loop32(c)
    want, ys = A.corrections(m, c.o.gposes, c.o.gposes_y)
    mine = A.corrections(m, got.gposes, dtype=F32)
    worst = 0.0
    for form in FORMS:
        A.check_outputs(form, "loop32/module", got, c)
        for s, (g, w, b, y) in enumerate(zip(mine, want, A.corrections_bars(form, c.x.shape[0], ys), ys)):
            for i in range(2):
                A.check(f"atlas corrections ({form})", f"loop32/module/{s}/{i}", g[i], w[i], b[i])
                worst = max(worst, ((g[i].double() - w[i]).abs() / (A.U * y[i])).max().item())
    print(f"module: fp32 restatement, corrections: worst |fp32 - fp64| / (u yardstick) {worst:.4f}")
    assert 0.25 * A.RESTATEMENT["corrections"] <= worst <= 1.25 * A.RESTATEMENT["corrections"]
    # the faults of the pose table reach the corrections: R for R^T cannot (gx only), x_local for x_world does
    bad = A.corrections(m, A.fault(7, c).gposes)
    bars = A.corrections_bars("split", c.x.shape[0], ys)
    assert any(bool(((b[i] - w[i]).abs() > bar[i]).any()) for b, w, bar in zip(bad, want, bars) for i in range(2))


@pytest.mark.parametrize("k", sorted(A.FAULTS))
def test_bars_reject_planted_faults(k):
    what, name = A.FAULTS[k]
    c = A.case(name)
    got = A.fault(k, c)
    for form in FORMS:
        assert A.rejected(form, got, c), f"fault {k} ({what}) passes every bar of case {name} ({form})"
    if k == 10:      # on the lonely runs themselves the fault cannot show: the other 63 rows are zero whatever divides them
        assert torch.equal(got.feat[64:192], c.o.feat[64:192])
