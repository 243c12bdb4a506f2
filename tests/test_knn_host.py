"""k nearest neighbours on the cell-list index (csrc/knn.hip), the part that needs no GPU: the exported symbols, every
argument check of the three entry points, the refusals of the ops, and the conditions that tests/test_knn.py relies on,
checked on the fixtures themselves."""
import ctypes

import numpy as np
import pytest
import torch

import icp_cases as ic
import knn_cases as kc
import nn_cases as nc

BADARG = 2001


def _plan(lo, hi, cell, n_tgt, max_rings=4):
    from miso_amd import _lib
    p = _lib.NnPlan()
    rc = _lib.load().miso_nn_plan((ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*hi), cell, n_tgt, max_rings, ctypes.byref(p))
    assert rc == 0
    return p


def test_knn_symbols_are_exported_and_bound():
    from miso_amd import _lib, ops
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("miso_nn_knn", "miso_nn_knn_all_pairs", "miso_nn_knn_normals"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert _lib.NN_KNN_MAX == 32 == ops.NN_KNN_MAX
    assert callable(ops.knn) and callable(ops.knn_all_pairs) and callable(ops.NearestIndex.knn)
    from miso_amd.grid_opt.utils import utils_ncd, utils_registration
    assert callable(utils_registration.estimate_normals) and callable(utils_ncd.align_mesh_to_ref)


def test_knn_entry_points_validate_arguments_without_gpu():
    """Malformed calls are refused before any launch (the pointers below are host arrays that a launch must never see)."""
    from miso_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    ptr = ctypes.c_void_p(ctypes.addressof(buf))
    off = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    assert ctypes.addressof(buf) % 16 == 0
    p = _plan((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 0.1, 10)
    pp, unplanned = ctypes.byref(p), ctypes.byref(_lib.NnPlan())
    broken = _lib.NnPlan.from_buffer_copy(p)
    broken.dims[0] = 1000                                               # dims no longer multiply to cells
    knn, pairs, normals = lib.miso_nn_knn, lib.miso_nn_knn_all_pairs, lib.miso_nn_knn_normals
    # (plan, workspace, src, ld, n, k, out_d2, out_idx, stats, stream)
    for k in (0, -1, 33, 1 << 20):
        assert knn(pp, ptr, ptr, 3, 8, k, ptr, ptr, ptr, None) == BADARG, k
        assert pairs(ptr, 3, 8, ptr, 3, 8, k, ptr, ptr, None) == BADARG, k
        assert normals(pp, ptr, ptr, 3, 8, k, ptr, ptr, None) == BADARG, k
    assert knn(None, ptr, ptr, 3, 8, 30, ptr, ptr, ptr, None) == BADARG
    assert knn(unplanned, ptr, ptr, 3, 8, 30, ptr, ptr, ptr, None) == BADARG
    assert knn(ctypes.byref(broken), ptr, ptr, 3, 8, 30, ptr, ptr, ptr, None) == BADARG
    assert knn(pp, None, ptr, 3, 8, 30, ptr, ptr, ptr, None) == BADARG
    assert knn(pp, off, ptr, 3, 8, 30, ptr, ptr, ptr, None) == BADARG                    # workspace alignment
    assert knn(pp, ptr, None, 3, 8, 30, ptr, ptr, ptr, None) == BADARG
    assert knn(pp, ptr, ptr, 2, 8, 30, ptr, ptr, ptr, None) == BADARG                    # ld < 3
    assert knn(pp, ptr, ptr, 3, -1, 30, ptr, ptr, ptr, None) == BADARG
    assert knn(pp, ptr, ptr, 3, 1 << 31, 30, ptr, ptr, ptr, None) == BADARG
    assert knn(pp, ptr, ptr, 3, 8, 30, None, ptr, ptr, None) == BADARG
    assert knn(pp, ptr, ptr, 3, 8, 30, ptr, None, ptr, None) == BADARG
    assert knn(pp, ptr, ptr, 3, 8, 30, ptr, ptr, None, None) == BADARG
    assert knn(pp, ptr, ptr, 3, 0, 30, ptr, ptr, None, None) == BADARG                   # stats even with n == 0
    # (tgt, ld_t, m, src, ld_s, n, k, out_d2, out_idx, stream)
    assert pairs(None, 3, 8, ptr, 3, 8, 30, ptr, ptr, None) == BADARG
    assert pairs(ptr, 3, 8, None, 3, 8, 30, ptr, ptr, None) == BADARG
    assert pairs(ptr, 2, 8, ptr, 3, 8, 30, ptr, ptr, None) == BADARG
    assert pairs(ptr, 3, 8, ptr, 2, 8, 30, ptr, ptr, None) == BADARG
    assert pairs(ptr, 3, -1, ptr, 3, 8, 30, ptr, ptr, None) == BADARG
    assert pairs(ptr, 3, 8, ptr, 3, -1, 30, ptr, ptr, None) == BADARG
    assert pairs(ptr, 3, 1 << 31, ptr, 3, 8, 30, ptr, ptr, None) == BADARG
    assert pairs(ptr, 3, 8, ptr, 3, 1 << 31, 30, ptr, ptr, None) == BADARG
    assert pairs(ptr, 3, 8, ptr, 3, 8, 30, None, ptr, None) == BADARG
    assert pairs(ptr, 3, 8, ptr, 3, 8, 30, ptr, None, None) == BADARG
    assert pairs(ptr, 3, 8, None, 3, 0, 30, None, None, None) == 0                       # n = 0: nothing to do
    # (plan, workspace, pts, ld, n, k, normals, counts, stream)
    assert normals(None, ptr, ptr, 3, 8, 30, ptr, ptr, None) == BADARG
    assert normals(unplanned, ptr, ptr, 3, 8, 30, ptr, ptr, None) == BADARG
    assert normals(ctypes.byref(broken), ptr, ptr, 3, 8, 30, ptr, ptr, None) == BADARG
    assert normals(pp, None, ptr, 3, 8, 30, ptr, ptr, None) == BADARG
    assert normals(pp, off, ptr, 3, 8, 30, ptr, ptr, None) == BADARG
    assert normals(pp, ptr, None, 3, 8, 30, ptr, ptr, None) == BADARG
    assert normals(pp, ptr, ptr, 2, 8, 30, ptr, ptr, None) == BADARG
    assert normals(pp, ptr, ptr, 3, -1, 30, ptr, ptr, None) == BADARG
    assert normals(pp, ptr, ptr, 3, 1 << 31, 30, ptr, ptr, None) == BADARG
    assert normals(pp, ptr, ptr, 3, 8, 30, None, ptr, None) == BADARG
    assert normals(pp, ptr, ptr, 3, 8, 30, ptr, None, None) == BADARG
    assert normals(pp, ptr, None, 3, 0, 30, None, None, None) == 0                       # n = 0: nothing to do


def test_knn_ops_refuse_cpu_tensors_and_bad_k():
    from miso_amd import ops
    from miso_amd.grid_opt.utils import utils_registration as reg
    a, b = torch.rand(10, 3), torch.rand(12, 3)
    for call in (lambda: ops.knn(a, b, 3), lambda: ops.knn_all_pairs(a, b, 3), lambda: reg.estimate_normals(b)):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()


def test_the_references_agree_on_ties_and_padding():
    """knn32 / knn64 themselves: the lattice's eight equidistant corners come out in index order, a duplicated row's first
    copy first, and rows without a match are padded."""
    D, I = kc.reference32("lattice", 7)
    assert (D == np.float32(3.0 / 256.0)).all() and (np.diff(I, axis=1) > 0).all()
    assert np.array_equal(I, kc.reference64("lattice", 7)[1])
    assert np.array_equal(I[:, 0], nc.reference("lattice")[1])
    D, I = kc.reference32("dup", 2)
    pair = D[:, 0] == D[:, 1]
    assert (I[:, 0] < I[:, 1])[pair].all()
    D, I = kc.reference32("single", 30)
    assert (I[:, 0] == 0).all() and (I[:, 1:] == -1).all() and np.isposinf(D[:, 1:]).all()
    D, I = kc.reference32("nan", 30)
    bad = ~np.isfinite(nc.case("nan")["src"]).all(axis=1)
    assert (I[bad] == -1).all() and np.isposinf(D[bad]).all() and (I[~bad] >= 0).all()
    assert not np.isin(I, [3, 77, 150, 151]).any()
    for name in ("empty", "nan_targets", "m0"):
        D, I = kc.reference32(name, 2)
        assert (I == -1).all() and np.isposinf(D).all()
    assert kc.reference32("n0", 30)[0].shape == (0, 30)
    for name in ("room", "crowd"):                                       # k = 1 is the 1-NN reference
        assert np.array_equal(kc.reference64(name, 1)[1][:, 0], nc.reference(name)[1])


def test_normals_fixture_meets_its_conditions():
    """icp_cases.fixture()'s 6 000 targets among themselves at k = 30.  Measured here: the fp32 and float64 neighbour sets
    are equal for all 6 000 queries, the smallest relative gap between the k-th and (k+1)-th true d2 is 1.33e-6, no fp32
    tie occurs inside a list, and 5 999 points have an eigen-gap >= 0.05.  Asserted: the set equality, and that at least
    99.9 % of the points are kept by the gap -- a cap on what the normals test may leave out, not a tolerance."""
    D, I, d32, i32 = kc.fixture_neighbours()
    assert np.array_equal(np.sort(I, axis=1), np.sort(i32, axis=1))
    assert (I[:, 0] == np.arange(6000)).all() and (D[:, 0] == 0.0).all()   # a point is its own first neighbour
    rel = (D[:, kc.K_NORMALS] - D[:, kc.K_NORMALS - 1]) / D[:, kc.K_NORMALS - 1]
    ties = int((np.diff(d32, axis=1) == 0).sum())
    _, counts, gaps = kc.fixture_normals()
    kept = float((gaps >= 0.05).mean())
    print(f"k-th / (k+1)-th gap: smallest {rel.min():.3e}; fp32 ties inside a list: {ties}; eigen-gap >= 0.05: {kept:.4%}")
    assert rel.min() > 0.0 and (counts == kc.K_NORMALS).all()
    assert kept >= 0.999


def test_the_default_index_finishes_the_fixture_in_its_rings():
    """The float64 ring rule at the default cell finishes every query of the fixture within max_rings = 4 for the NEAREST
    neighbour (nn_cases.ring_rule64), and the k-th neighbour lies within 4 default cells, so that ring 4's box, whose open
    faces are at least 4 cells away, holds the whole list: the default index does not exercise the all-pairs kernel here, so tests/test_knn.py forces it (max_rings = 0 on `room`, `far`, `segments`)."""
    from miso_amd import ops
    t = ic.fixture()["tgt"]
    cell = ops.nn_default_cell(t.min(axis=0), t.max(axis=0), len(t))
    rings, _ = nc.ring_rule64(t[:500], t, cell, ops.NN_MAX_RINGS)
    assert (rings <= ops.NN_MAX_RINGS).all()
    D = kc.fixture_neighbours()[0]
    assert np.sqrt(D[:, kc.K_NORMALS - 1]).max() < 4.0 * cell
    c = nc.case("room")                                                  # what the forced fallback relies on
    rings, _ = nc.ring_rule64(c["src"], c["tgt"], 0.02, 0)
    assert (rings > 0).sum() >= 1000
