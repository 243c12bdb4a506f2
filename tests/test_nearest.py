"""Exact 1-nearest-neighbour (csrc/nn.hip, ops.NearestIndex / nearest / nearest_all_pairs).

CPU: the fixtures of tests/nn_cases.py against the float64 ring rule, the host plan, the workspace size, the refusals
and the exported symbols.  GPU: the index route and the all-pairs route agree bit for bit on every case, both are the
float64 nearest neighbour within the rounding of five fp32 operations, ties go to the lowest index, the counters add
up, and a side stream and a replayed graph return the eager bits."""
import ctypes

import numpy as np
import pytest
import torch

import nn_cases as nc

BADARG, TOOLARGE = 2001, 2003
CAP = 1 << 24


def _plan(lo, hi, cell, n_tgt, max_rings=4):
    from miso_amd import _lib
    lib = _lib.load()
    p = _lib.NnPlan()
    rc = lib.miso_nn_plan((ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*hi), cell, n_tgt, max_rings, ctypes.byref(p))
    return rc, p


# --------------------------------------------------------------------------- CPU
def test_fixtures_meet_their_conditions_in_float64():
    """What the GPU tests rely on, checked on the clouds themselves: `room` leaves its 103 far queries (and at most 10 % of
    all) past ring 4, `far` leaves every query, and wherever the ring rule finishes its answer is the all-pairs one."""
    for name in ("room", "far", "lattice", "faces", "crowd", "dup"):
        c = nc.case(name)
        rings, idx = nc.ring_rule64(c["src"], c["tgt"], c["cell"], c["max_rings"])
        D, I = nc.reference(name)
        fin = rings <= c["max_rings"]
        assert (idx[fin] == I[fin]).all(), name
        left = int((~fin).sum())
        if name == "room":
            assert 103 <= left <= 205 and not fin[:103].any()
        elif name == "far":
            assert left == 700 == len(rings)
        elif name == "lattice":
            assert left == 0
    D, I = nc.reference("lattice")
    assert (D == 3.0 / 256.0).all()                                     # eight targets tie exactly
    t = nc.case("lattice")["tgt"].astype(np.float64)
    s = nc.case("lattice")["src"].astype(np.float64)
    ties = (((s[:, None, :] - t[None, :, :]) ** 2).sum(axis=2) == 3.0 / 256.0).sum(axis=1)
    assert (ties == 8).all()
    D, I = nc.reference("dup")
    assert (I < 600).all()                                              # the first copy of a duplicated row
    D, I = nc.reference("nan")
    bad = ~np.isfinite(nc.case("nan")["src"]).all(axis=1)
    assert bad.sum() == 4 and (I[bad] == -1).all() and (I[~bad] >= 0).all()
    assert (nc.reference("empty")[1] == -1).all() and (nc.reference("nan_targets")[1] == -1).all()


def test_stop_rule_without_slack_errs_on_straddle_and_the_slack_repairs_it():
    """`straddle` in the kernel's own fp32 arithmetic (nn_cases.ring0_fp32): the bare rule best <= g finishes after ring 0
    on the wrong neighbour, by far more than the 2^-19 the GPU test allows; with the slack of ring_finished no query of
    the fixture stops there (ring 1 holds A).  `faces` (all coordinates near 37 m) has no such query: see its docstring."""
    c = nc.case("straddle")
    D, I = nc.reference("straddle")
    groups = c["groups"]
    assert len(groups) >= 10 and (I[groups[:, 0]] == groups[:, 1]).all()           # A is the nearest everywhere
    bare_fin, bare_idx = nc.ring0_fp32(c, slack=False)
    wrong = bare_fin & (bare_idx != I)
    assert wrong.sum() >= 10 and (bare_idx[wrong] == groups[wrong, 2]).all()        # ... and the bare rule answers B
    Dj = nc.true_d2(c["src"], c["tgt"], bare_idx)
    assert (Dj[wrong] > D[wrong] * (1.0 + 1e-3)).all()
    fin, idx = nc.ring0_fp32(c, slack=True)
    assert not (fin & (idx != I)).any() and not fin[wrong].any()
    rings, idx64 = nc.ring_rule64(c["src"], c["tgt"], c["cell"], c["max_rings"])
    assert (rings <= 1).all() and (idx64 == I).all()
    f = nc.case("faces")
    bare_fin, bare_idx = nc.ring0_fp32(f, slack=False)
    assert not (bare_fin & (bare_idx != nc.reference("faces")[1])).any()


def test_plan_dims_and_cell():
    c = nc.case("room")
    lo, hi = c["tgt"].min(axis=0), c["tgt"].max(axis=0)
    rc, p = _plan(lo, hi, 0.1, len(c["tgt"]))
    assert rc == 0 and tuple(p.dims) == (41, 31, 26) and p.cells == 41 * 31 * 26 and p.cell == np.float32(0.1)
    assert tuple(nc.plan64(c["tgt"], 0.1)[2]) == (41, 31, 26)
    assert p.n_tgt == 3001 and p.max_rings == 4 and tuple(p.bound_min) == tuple(lo)
    assert p.coord_mag >= 4.0 + 4.1                                     # largest |coordinate| + largest extent
    c = nc.case("capped")
    lo, hi = c["tgt"].min(axis=0), c["tgt"].max(axis=0)
    rc, p = _plan(lo, hi, 0.05, len(c["tgt"]))
    assert rc == 0 and p.cell > 0.05 and p.cells <= CAP and p.cells == p.dims[0] * p.dims[1] * p.dims[2]
    assert p.cell == np.float32(0.05) * 128 and tuple(p.dims) == (157, 157, 157)       # the first doubling that fits
    assert (nc.plan64(c["tgt"], 0.05)[2] == 157).all()
    rc, p = _plan((0.0, 0.0, 1.5), (2.0, 1.0, 1.5), 0.25, 100)          # a flat cloud
    assert rc == 0 and tuple(p.dims) == (9, 5, 1)
    rc, p = _plan((1.0, 1.0, 1.0), (1.0, 1.0, 1.0), 0.25, 1)
    assert rc == 0 and tuple(p.dims) == (1, 1, 1) and p.cells == 1
    rc, p = _plan((0.0,) * 3, (0.0,) * 3, 0.25, 0)                      # no target: a valid plan
    assert rc == 0 and p.n_tgt == 0


def test_workspace_bytes_follow_the_formula():
    from miso_amd import _lib
    lib = _lib.load()
    a256 = lambda v: (v + 255) // 256 * 256                             # noqa: E731
    for lo, hi, cell, m in (((0, 0, 0), (4, 3, 2.5), 0.1, 3001), ((0, 0, 0), (1, 1, 1), 0.01, 1), ((0, 0, 0), (0, 0, 0), 1.0, 77)):
        rc, p = _plan(lo, hi, cell, m)
        assert rc == 0
        want = (a256((p.cells + 1) * 4) + a256(1024 * 4) + a256(_lib.NN_MAX_CHUNKS * 4) + a256(_lib.NN_CHUNK * 4) +
                a256(m * 16))
        assert lib.miso_nn_workspace_bytes(ctypes.byref(p)) == want
    assert lib.miso_nn_workspace_bytes(None) == 0
    p = _lib.NnPlan()                                                   # not written by miso_nn_plan
    assert lib.miso_nn_workspace_bytes(ctypes.byref(p)) == 0
    assert _lib.NN_MAX_CELLS == CAP


def test_nn_entry_points_validate_arguments_without_gpu():
    """Malformed calls are refused before any launch (the pointers below are host arrays that a launch must never see)."""
    from miso_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    ptr = ctypes.c_void_p(ctypes.addressof(buf))
    assert ctypes.addressof(buf) % 16 == 0
    lo, hi = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    for bad in (0.0, -0.1, float("inf"), float("nan")):
        assert _plan(lo, hi, bad, 10)[0] == BADARG, bad
    assert _plan(lo, (1.0, -1.0, 1.0), 0.1, 10)[0] == BADARG             # max < min
    assert _plan(lo, (1.0, float("nan"), 1.0), 0.1, 10)[0] == BADARG
    assert _plan(lo, (1.0, float("inf"), 1.0), 0.1, 10)[0] == BADARG
    assert _plan(lo, hi, 0.1, -1)[0] == BADARG
    assert _plan(lo, hi, 0.1, 10, max_rings=-1)[0] == BADARG
    assert _plan(lo, hi, 0.1, 10, max_rings=65)[0] == BADARG and _plan(lo, hi, 0.1, 10, max_rings=64)[0] == 0
    assert _plan(lo, hi, 0.1, 1 << 31)[0] == TOOLARGE
    f3 = (ctypes.c_float * 3)(0, 0, 0)
    assert lib.miso_nn_plan(None, f3, 0.1, 10, 4, ctypes.byref(_lib.NnPlan())) == BADARG
    assert lib.miso_nn_plan(f3, f3, 0.1, 10, 4, None) == BADARG
    rc, p = _plan(lo, hi, 0.1, 10)
    assert rc == 0
    pp = ctypes.byref(p)
    build, query, pairs = lib.miso_nn_build, lib.miso_nn_query, lib.miso_nn_all_pairs
    assert build(None, ptr, 3, ptr, None) == BADARG
    assert build(pp, None, 3, ptr, None) == BADARG
    assert build(pp, ptr, 3, None, None) == BADARG
    assert build(pp, ptr, 2, ptr, None) == BADARG                       # ld < 3
    assert build(pp, ptr, 3, ctypes.c_void_p(ctypes.addressof(buf) + 4), None) == BADARG       # workspace alignment
    assert build(ctypes.byref(_lib.NnPlan()), ptr, 3, ptr, None) == BADARG                     # a plan nobody planned
    assert query(None, ptr, ptr, 3, 8, ptr, ptr, ptr, None) == BADARG
    assert query(pp, None, ptr, 3, 8, ptr, ptr, ptr, None) == BADARG
    assert query(pp, ptr, None, 3, 8, ptr, ptr, ptr, None) == BADARG
    assert query(pp, ptr, ptr, 2, 8, ptr, ptr, ptr, None) == BADARG
    assert query(pp, ptr, ptr, 3, -1, ptr, ptr, ptr, None) == BADARG
    assert query(pp, ptr, ptr, 3, 8, None, ptr, ptr, None) == BADARG
    assert query(pp, ptr, ptr, 3, 8, ptr, None, ptr, None) == BADARG
    assert query(pp, ptr, ptr, 3, 8, ptr, ptr, None, None) == BADARG
    assert query(pp, ptr, ptr, 3, 1 << 31, ptr, ptr, ptr, None) == TOOLARGE
    broken = _lib.NnPlan.from_buffer_copy(p)
    broken.dims[0] = 1000                                               # dims no longer multiply to cells
    assert query(ctypes.byref(broken), ptr, ptr, 3, 8, ptr, ptr, ptr, None) == BADARG
    assert pairs(None, 3, 8, ptr, 3, 8, ptr, ptr, None) == BADARG
    assert pairs(ptr, 3, 8, None, 3, 8, ptr, ptr, None) == BADARG
    assert pairs(ptr, 2, 8, ptr, 3, 8, ptr, ptr, None) == BADARG
    assert pairs(ptr, 3, 8, ptr, 2, 8, ptr, ptr, None) == BADARG
    assert pairs(ptr, 3, -1, ptr, 3, 8, ptr, ptr, None) == BADARG
    assert pairs(ptr, 3, 8, ptr, 3, -1, ptr, ptr, None) == BADARG
    assert pairs(ptr, 3, 8, ptr, 3, 8, None, ptr, None) == BADARG
    assert pairs(ptr, 3, 8, ptr, 3, 8, ptr, None, None) == BADARG
    assert pairs(ptr, 3, 1 << 31, ptr, 3, 8, ptr, ptr, None) == TOOLARGE


def test_nn_symbols_are_exported_and_bound():
    from miso_amd import _lib, ops
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("miso_nn_plan", "miso_nn_workspace_bytes", "miso_nn_build", "miso_nn_query", "miso_nn_all_pairs"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert _lib.STRUCTS["miso_nn_plan_t"] is _lib.NnPlan
    assert callable(ops.nearest) and callable(ops.nearest_all_pairs) and callable(ops.NearestIndex.query)


def test_nearest_refuses_cpu_tensors():
    from miso_amd import ops
    a, b = torch.rand(10, 3), torch.rand(12, 3)
    for call in (lambda: ops.nearest(a, b), lambda: ops.nearest_all_pairs(a, b), lambda: ops.NearestIndex(b)):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()


def test_default_cell_rule():
    from miso_amd import ops
    # 59 m^2 of box surface, 59 000 points: a spacing of 1 / sqrt(1000) m
    cell = ops.nn_default_cell((0, 0, 0), (4, 3, 2.5), 59000)
    assert cell == pytest.approx(ops.NN_CELL_SPACINGS * (59.0 / 59000) ** 0.5)
    assert ops.nn_default_cell((0, 0, 0), (2, 0, 0), 100) == pytest.approx(ops.NN_CELL_SPACINGS * 0.02)     # a line
    assert ops.nn_default_cell((1, 1, 1), (1, 1, 1), 5) == 1.0                                                # a point


# --------------------------------------------------------------------------- GPU
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_results = {}


def _run(name):
    """(index route d2, idx, stats; all-pairs route d2, idx) of a case as numpy arrays, computed once"""
    if name not in _results:
        from miso_amd import ops
        c = nc.case(name)
        src, tgt = _dev(c["src"]), _dev(c["tgt"])
        d2, idx, stats = ops.NearestIndex(tgt, cell=c["cell"], max_rings=c["max_rings"]).query(src)
        e2, edx = ops.nearest_all_pairs(src, tgt)
        torch.cuda.synchronize()
        _results[name] = tuple(t.cpu().numpy() for t in (d2, idx, stats, e2, edx))
    return _results[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", nc.NAMES)
def test_index_and_all_pairs_agree_bit_for_bit(name):
    d2, idx, stats, e2, edx = _run(name)
    n = len(nc.case(name)["src"])
    assert d2.shape == (n,) and idx.shape == (n,) and d2.dtype == np.float32 and idx.dtype == np.int64
    assert (d2.view(np.int32) == e2.view(np.int32)).all()
    assert (idx == edx).all()
    assert int(stats[0]) + int(stats[1]) == n


@pytest.mark.gpu
@pytest.mark.parametrize("name", nc.NAMES)
def test_answer_is_the_float64_nearest_neighbour(name):
    """j = the returned index, D_j its true squared distance, D* the true minimum (float64 on the fp32 inputs).  The kernel
    orders fp32 values that are each within 5 * 2^-24 of the truth: D_j <= D* (1 + 2^-19); the returned d2 is within
    2^-21 of D_j (three differences, three squares, two sums: five roundings on a path)."""
    d2, idx, _, _, _ = _run(name)
    c = nc.case(name)
    D, I = nc.reference(name)
    has = I >= 0
    assert ((idx >= 0) == has).all()
    assert (idx[~has] == -1).all() and np.isposinf(d2[~has]).all()
    assert (idx[has] < len(c["tgt"])).all()
    Dj = nc.true_d2(c["src"], c["tgt"], idx)
    assert (Dj[has] <= D[has] * (1.0 + 2.0 ** -19)).all()
    assert np.isfinite(d2[has]).all()
    assert (np.abs(d2[has].astype(np.float64) - Dj[has]) <= 2.0 ** -21 * Dj[has]).all()


@pytest.mark.gpu
def test_ties_go_to_the_lowest_index_and_rows_without_a_match_get_none():
    for name in ("lattice", "dup"):
        d2, idx, _, _, edx = _run(name)
        D, I = nc.reference(name)
        assert (idx == I).all() and (edx == I).all(), name
    d2, idx, _, _, _ = _run("lattice")
    assert (d2 == np.float32(3.0 / 256.0)).all()
    d2, idx, _, _, _ = _run("empty")
    assert np.isposinf(d2).all() and (idx == -1).all()
    d2, idx, _, _, _ = _run("nan_targets")
    assert np.isposinf(d2).all() and (idx == -1).all()
    d2, idx, _, _, _ = _run("nan")
    bad = ~np.isfinite(nc.case("nan")["src"]).all(axis=1)
    assert np.isposinf(d2[bad]).all() and (idx[bad] == -1).all()
    assert np.isfinite(d2[~bad]).all() and (idx[~bad] >= 0).all()
    assert not np.isin(idx, [3, 77, 150, 151]).any()                    # the non-finite targets are nobody's neighbour


@pytest.mark.gpu
def test_counters():
    for name in nc.NAMES:
        stats = _run(name)[2]
        assert int(stats[0]) + int(stats[1]) == len(nc.case(name)["src"]), name
    assert 103 <= int(_run("room")[2][1]) <= 205
    assert int(_run("far")[2][1]) == 700
    assert int(_run("lattice")[2][1]) == 0
    assert int(_run("empty")[2][1]) == 0
    assert int(_run("segments")[2][1]) >= 230                           # the shifted queries reach the second kernel


@pytest.mark.gpu
def test_strided_view_is_read_in_place():
    from miso_amd import ops
    c = nc.case("n257")
    src4 = torch.zeros(257, 4, device="cuda")
    tgt4 = torch.full((1031, 4), 7.0, device="cuda")
    src4[:, :3], tgt4[:, :3] = _dev(c["src"]), _dev(c["tgt"])
    ix = ops.NearestIndex(tgt4[:, :3], cell=c["cell"], max_rings=c["max_rings"])
    assert ix.tgt.data_ptr() == tgt4.data_ptr()                          # no copy
    d2, idx, _ = ix.query(src4[:, :3])
    e2, edx = ops.nearest_all_pairs(src4[:, :3], tgt4[:, :3])
    want = _run("n257")
    for got in ((d2, idx), (e2, edx)):
        assert (got[0].cpu().numpy().view(np.int32) == want[0].view(np.int32)).all() and (got[1].cpu().numpy() == want[1]).all()


@pytest.mark.gpu
def test_two_calls_a_side_stream_and_a_replayed_graph_return_the_same_bits():
    """The build reads the bounds back, so it stays outside the capture; the query replays."""
    from miso_amd import ops
    c = nc.case("room")
    src, tgt = _dev(c["src"]), _dev(c["tgt"])
    want = _run("room")
    ix = ops.NearestIndex(tgt, cell=c["cell"], max_rings=c["max_rings"])

    def same(d2, idx, stats):
        torch.cuda.synchronize()
        return ((d2.cpu().numpy().view(np.int32) == want[0].view(np.int32)).all() and (idx.cpu().numpy() == want[1]).all()
                and (stats.cpu().numpy() == want[2]).all())

    assert same(*ix.query(src))                                          # a second index, a second call
    assert same(*ix.query(src))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = ops.NearestIndex(tgt, cell=c["cell"], max_rings=c["max_rings"]).query(src)
    side.synchronize()
    assert same(*out)
    out = (torch.empty(len(c["src"]), device="cuda"), torch.empty(len(c["src"]), device="cuda", dtype=torch.int64),
           torch.empty(2, device="cuda", dtype=torch.int32))
    ix.query(src, out=out)                                               # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ix.query(src, out=out)
    for _ in range(2):
        for t in out:
            t.zero_()
        graph.replay()
        assert same(*out)


@pytest.mark.gpu
def test_nearest_picks_a_route_by_size_and_both_give_the_same_bits(monkeypatch):
    from miso_amd import ops
    c = nc.case("crowd")
    src, tgt = _dev(c["src"]), _dev(c["tgt"])
    want = _run("crowd")
    assert len(c["src"]) * len(c["tgt"]) < ops.NN_ALL_PAIRS_BELOW
    small = ops.nearest(src, tgt)                                        # the all-pairs route
    monkeypatch.setattr(ops, "NN_ALL_PAIRS_BELOW", 0)
    large = ops.nearest(src, tgt)                                        # the index route, default cell and rings
    for d2, idx in (small, large):
        assert (d2.cpu().numpy().view(np.int32) == want[0].view(np.int32)).all() and (idx.cpu().numpy() == want[1]).all()


@pytest.mark.gpu
def test_more_queries_than_one_chunk():
    """N = 2^20 + 777 queries run as two chunks (their own list counter, the list reused): the index route and the
    all-pairs route agree bit for bit, the counters add up, both chunks list queries, and 3000 queries around the chunk
    border and at both ends are the float64 neighbour."""
    from miso_amd import _lib, ops
    n = _lib.NN_CHUNK + 777
    rng = np.random.default_rng(1300)
    tgt = nc.box_surface(rng, 2003, (1.0, 1.0, 1.0)).astype(np.float32)
    src = rng.random((n, 3), dtype=np.float32)
    far = np.concatenate([np.arange(0, n, 4099), np.arange(_lib.NN_CHUNK - 50, _lib.NN_CHUNK + 50)])
    src[far] += np.float32(2.0)
    s, t = _dev(src), _dev(tgt)
    d2, idx, stats = ops.NearestIndex(t, cell=0.05, max_rings=3).query(s)
    e2, edx = ops.nearest_all_pairs(s, t)
    assert torch.equal(d2.view(torch.int32), e2.view(torch.int32)) and torch.equal(idx, edx)
    stats = stats.cpu().numpy()
    assert int(stats[0]) + int(stats[1]) == n and int(stats[1]) >= len(np.unique(far))
    pick = np.unique(np.concatenate([np.arange(1000), np.arange(_lib.NN_CHUNK - 500, _lib.NN_CHUNK + 500), np.arange(n - 1000, n), far]))
    D, I = nc.all_pairs64(src[pick], tgt)
    got_i, got_d = idx.cpu().numpy()[pick], d2.cpu().numpy()[pick].astype(np.float64)
    Dj = nc.true_d2(src[pick], tgt, got_i)
    assert (got_i >= 0).all() and (Dj <= D * (1.0 + 2.0 ** -19)).all() and (np.abs(got_d - Dj) <= 2.0 ** -21 * Dj).all()
