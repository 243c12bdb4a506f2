"""CPU-side anchors of the grid Adam step: the step scalars and the table-length rule through the loaded library, and
the fp32 restatement the GPU tests compare bits with (adam_cases.step32) tied to float64 -- to the same formula with a
derived rounding bound, and through it to torch.optim.Adam's step from float64 hyper-parameters."""
import ctypes
import math

import numpy as np
import pytest
import torch

import adam_cases as A

U = A.U


def _rows(lr, b1, b2, eps, first, count):
    from miso_amd import _lib
    host = torch.empty((count, 6), dtype=torch.float32)
    assert _lib.load().miso_adam_scalars_table(lr, b1, b2, eps, first, count, ctypes.c_void_p(host.data_ptr())) == 0
    return host.numpy().copy()


def test_step_scalars_are_the_formula_bit_for_bit():
    """miso_adam_scalars_table at every HYPERS x STEPS = float32 of {1 - b1, b2, 1 - b2, -(lr / (1 - b1^t)),
    sqrt(1 - b2^t), eps} in Python floats: both sides are IEEE double arithmetic around libm's pow and sqrt, so every
    column is asserted bit for bit (none needed an ulp here)."""
    for lr, b1, b2, eps in A.HYPERS:
        for t in A.STEPS:
            got = _rows(lr, b1, b2, eps, t, 1)[0]
            want = A.scalars_of(lr, b1, b2, eps, t)
            assert got.view(np.int32).tolist() == want.view(np.int32).tolist(), ((lr, b1, b2, eps), t, got, want)
            assert np.isfinite(got).all() and got[3] < 0 and 0 < got[4] <= 1


def _constant_from(table):
    """The first 1-based step from which every row of ``table`` equals its last one."""
    differs = np.flatnonzero((table.view(np.int32) != table.view(np.int32)[-1]).any(1))
    return 1 if differs.size == 0 else int(differs[-1]) + 2


def test_table_length_rule_reaches_the_constant_row():
    """AdamDeviceStep sizes its table by ops.adam_table_rows and lets a count past the table read the last row: that
    row must be the row of every later step.  The library's row at step `rows` equals its rows at rows + 1, 2 rows,
    10^6 and 10^9, and the first step from which the row no longer changes is <= rows -- for the defaults step 16 628
    of 20 777 rows."""
    from miso_amd import ops
    first_constant = {}
    for lr, b1, b2, eps in A.HYPERS:
        rows = ops.adam_table_rows(b1, b2)
        assert rows is not None and 64 <= rows <= ops.AdamDeviceStep.MAX_ROWS
        table = _rows(lr, b1, b2, eps, 1, rows)
        last = table[-1].view(np.int32).tolist()
        for later in (rows + 1, 2 * rows, 10 ** 6, 10 ** 9):
            if later >= rows:
                assert _rows(lr, b1, b2, eps, later, 1)[0].view(np.int32).tolist() == last, ((b1, b2), later)
        first_constant[(b1, b2)] = _constant_from(table)
        assert first_constant[(b1, b2)] <= rows
        # by the formula alone: the same figure from Python floats
        want = np.stack([A.scalars_of(lr, b1, b2, eps, t) for t in range(1, rows + 1)])
        assert _constant_from(want) == first_constant[(b1, b2)]
    assert ops.adam_table_rows(0.9, 0.999) == 20777 and first_constant[(0.9, 0.999)] == 16628
    assert ops.adam_table_rows(0.0, 0.0) == 64 and ops.adam_table_rows(0.9, 1.0) is None
    for b1, b2 in ((0.9, 1.0), (1.0, 0.999), (0.9, 0.999999)):          # beta = 1; a table above MAX_ROWS
        with pytest.raises(ValueError, match="step-scalar table"):
            ops.AdamDeviceStep(1e-3, b1, b2, 1e-8, "cpu")


def test_layouts_put_every_value_class_on_every_path():
    """The rotations of adam_cases.layout together put every (gradient value, state) class of EDGE on the float4 path
    and on the ragged end of the flag-driven forms and on the dense float4 path, every gradient value on the dense
    numel % 4 tail, and every chunk role (woken by one subnormal, asleep under -0, stepped before) on the slab path,
    the ragged end and the partial last chunk."""
    every = set(range(A.N_CLASSES))
    seen = A.coverage(A.N_ACTIVE, dense=False)
    assert seen["slab"] == every and seen["ragged"] == every
    seen = A.coverage(A.N_DENSE, dense=True)
    assert seen["vec"] == every and {c // len(A.STATES) for c in seen["tail"]} == set(range(len(A.G_VALUES)))
    nslab_chunks = A.N_ACTIVE // A.SLAB * 4
    where = {"slab": set(), "ragged": set(), "partial": set()}
    for rot in range(A.N_ROT):
        L = A.layout(A.N_ACTIVE, rot)
        where["slab"] |= set(L.role[:nslab_chunks])
        where["ragged"] |= set(L.role[nslab_chunks:-1])
        where["partial"].add(L.role[-1])
        asleep = ~L.stepped
        assert (L.role[asleep] == "Z").all() and L.stepped[L.role != "Z"].all()
        single = L.role == "S"
        assert (L.active[single] == 0).all() and L.nonzero[single].all()
        g = L.g.copy()
        g.resize(L.nchunks * A.CHUNK)
        for c in np.flatnonzero(single):
            assert np.count_nonzero(g[c * A.CHUNK:(c + 1) * A.CHUNK]) == 1
    assert all(s == set("EZWS") for s in where.values()), where
    assert A.EDGE.size == len(A.G_VALUES) * len(A.STATES) * len(A.P_VALUES) and 0 < A.EDGE_FINITE.size < A.EDGE.size


def test_step32_lies_within_the_float64_bound_and_float64_is_adam():
    """On every record of EDGE_FINITE at every HYPERS x STEPS (no case left out):
    * step32 lies within step64's derived bound of step64's value, in p, m and v;
    * step64 (the kernel's formula from the fp32 table row) lies within 6 u relative of step_true64 (torch.optim.Adam in
      float64 from float64 hyper-parameters) in m and v, and in p within 6 u |r| + 2 u |r| (sqrt(v) / bc) / den: the six
      scalar roundings at u each, bc2_sqrt's and eps's reaching p through the denominator.  (Both sides are float64
      evaluations: 8 of their own roundings, 2^-53 of the operands each, are allowed on top.)"""
    E = A.EDGE_FINITE
    p, g, m, v = E["p"], E["g"], E["m"], E["v"]
    D = 2.0 ** -53
    n_checked = 0
    for hyper in A.HYPERS:
        for t in A.STEPS:
            sc = A.scalars_of(*hyper, t)
            got = A.step32(p, g, m, v, sc)
            val, err = A.step64(p, g, m, v, sc)
            for name, a, b, e in zip("pmv", got, val, err):
                assert np.isfinite(a).all() and np.isfinite(b).all()
                bad = np.flatnonzero(~(np.abs(a.astype(np.float64) - b) <= e))
                assert bad.size == 0, (name, hyper, t, E[bad[:4]], a[bad[:4]], b[bad[:4]], e[bad[:4]])
            pt, mt, vt, r, share = A.step_true64(p, g, m, v, t, *hyper)
            p64, m64, v64 = val
            m_in, v_in = np.abs(m.astype(np.float64)), v.astype(np.float64)
            g_abs = np.abs(g.astype(np.float64))
            bad = np.flatnonzero(~(np.abs(m64 - mt) <= 6 * U * np.abs(mt) + 8 * D * (m_in + g_abs)))
            assert bad.size == 0, ("m", hyper, t, E[bad[:4]], m64[bad[:4]], mt[bad[:4]])
            bad = np.flatnonzero(~(np.abs(v64 - vt) <= 6 * U * vt + 8 * D * vt))
            assert bad.size == 0, ("v", hyper, t, E[bad[:4]], v64[bad[:4]], vt[bad[:4]])
            margin = 6 * U * np.abs(r) + 2 * U * np.abs(r) * share + 8 * D * (np.abs(p.astype(np.float64)) + np.abs(r))
            bad = np.flatnonzero(~(np.abs(p64 - pt) <= margin))
            assert bad.size == 0, ("p", hyper, t, E[bad[:4]], p64[bad[:4]], pt[bad[:4]], margin[bad[:4]])
            n_checked += E.size
    assert n_checked == A.EDGE_FINITE.size * len(A.HYPERS) * len(A.STEPS)


def test_tracker_restatement_is_step32():
    """tracker_cases.adam32, the pose Adam's fp32 restatement, is step32 at betas above 0.5."""
    import tracker_cases
    E = A.EDGE_FINITE
    for lr, b1, b2, eps in (A.HYPERS[0], A.HYPERS[1], A.HYPERS[4]):
        for t in (1, 1000):
            want = A.step32(E["p"], E["g"], E["m"], E["v"], A.scalars_of(lr, b1, b2, eps, t))
            got = tracker_cases.adam32(torch.from_numpy(E["p"].copy()), torch.from_numpy(E["g"].copy()),
                                       torch.from_numpy(E["m"].copy()), torch.from_numpy(E["v"].copy()), t, lr, (b1, b2), eps)
            for a, b in zip(got, want):
                assert np.array_equal(a.numpy().astype(np.float32).view(np.int32), b.view(np.int32))
