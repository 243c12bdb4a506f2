"""Inputs and the float64 reference for the mapping-loss tests (tests/test_mapping_loss.py): the pointwise rule of
map_loss_one (csrc/common.hpp) restated in numpy, generated label batches that PLANT every branch point of the rule, and
the rounding bounds that follow from the structure of the kernels' sums.  Nothing here touches the library; every batch
is generated, none is stored."""
import numpy as np

F32 = np.float32
U = 2.0 ** -24                       # unit roundoff of fp32 (round to nearest: |fl(x) - x| <= U |x|)
W_SDF, W_FS = 2.0, 0.5               # term weights of the tests: powers of two, so they add no rounding


def gamma(k):
    """Relative error of a product of k correctly rounded factors, |prod (1 + d_i) - 1| <= k U / (1 - k U)."""
    return k * U / (1.0 - k * U)


# --------------------------------------------------------------------------- the rule
def _cols(pred, target, valid, sign, weight):
    s = np.ascontiguousarray(np.asarray(pred, dtype=F32).reshape(-1))
    n = len(s)
    t = np.asarray(target, dtype=F32).reshape(-1)
    v = np.ones(n, dtype=F32) if valid is None else np.asarray(valid, dtype=F32).reshape(-1)
    f = np.zeros(n, dtype=F32) if sign is None else np.asarray(sign, dtype=F32).reshape(-1)
    w = np.ones(n, dtype=F32) if weight is None else np.asarray(weight, dtype=F32).reshape(-1)
    assert len(t) == len(v) == len(f) == len(w) == n
    return s, t, v, f, w


def decisions(pred, target, valid, sign, trunc):
    """The branch decisions of the rule, each ONE IEEE fp32 operation on the given bits (a subtraction, a max, a
    comparison: nothing a compiler can contract), so numpy and the device agree on them bit for bit.
    -> d, up, lo (fp32) and the masks is_valid, is_free."""
    s, t, v, f, _ = _cols(pred, target, valid, sign, None)
    d = s - t
    up = np.maximum(d, F32(0))
    lo = np.maximum(F32(trunc) - s, F32(0))          # trunc rounded to fp32 first, as the C ABI's float does
    return d, up, lo, v == F32(1), f == F32(1)


def loss_rule(pred, target, valid, sign, weight, loss_type, w_sdf, w_fs, trunc, n_mean=None):
    """-> (terms[2], g_sdf (n), g_fs (n)) in float64: the two weighted means and their derivatives w.r.t. pred.
    Decisions in fp32 (decisions()); values and sums in float64 on the exactly converted inputs.  None columns: every
    row valid, no free-space row, weight 1.  n_mean: the divisor of the means (the live rows of a padded batch)."""
    s, t, v, f, w = _cols(pred, target, valid, sign, weight)
    n = len(s)
    div = float(n if n_mean is None else n_mean)
    d32, up32, lo32, is_valid, is_free = decisions(s, t, v, f, trunc)
    is_free = is_free & (w_fs > 0)
    s64, t64, w64 = s.astype(np.float64), t.astype(np.float64), w.astype(np.float64)
    d = s64 - t64
    if loss_type == "L1":
        per, slope = np.abs(d), (d32 > 0).astype(np.float64) - (d32 < 0).astype(np.float64)      # abs'(0) = 0
    else:
        assert loss_type == "L2"
        per, slope = d * d, 2.0 * d
    t_sdf = np.where(is_valid, w64 * per, 0.0)
    g_sdf = np.where(is_valid, w_sdf * w64 * slope, 0.0) / div
    up, lo = np.maximum(d, 0.0), np.maximum(float(F32(trunc)) - s64, 0.0)
    t_fs = np.where(is_free, np.maximum(up, lo), 0.0)
    # a tie of the maximum carries half of each side's slope, +1/2 - 1/2 = 0; relu'(0) = 0
    g_fs = np.where(is_free, w_fs * ((up32 > lo32).astype(np.float64) - (lo32 > up32).astype(np.float64)), 0.0) / div
    terms = np.array([w_sdf * t_sdf.sum() / div, w_fs * t_fs.sum() / div])
    return terms, g_sdf, g_fs


def abs_term_sums(pred, target, valid, sign, weight, loss_type, w_fs, trunc):
    """sum_i |term_i| of the two unweighted sums (what the rounding bound of a sum is relative to)."""
    terms, _, _ = loss_rule(pred, target, valid, sign, weight, loss_type, 1.0, 1.0 if w_fs > 0 else 0.0, trunc, n_mean=1)
    return terms                       # every term is non-negative


def classify(pred, target, valid, sign, trunc):
    """Masks of the branch classes a batch holds, from decisions()."""
    d, up, lo, is_valid, is_free = decisions(pred, target, valid, sign, trunc)
    _, _, v, f, _ = _cols(pred, target, valid, sign, None)
    return {
        "d0": is_valid & (d == 0),
        "tie_pos": is_free & (up == lo) & (lo > 0),
        "tie_zero": is_free & (up == lo) & (lo == 0),
        "up_gt": is_free & (up > lo),
        "lo_gt": is_free & (lo > up),
        "valid_out": ~is_valid,                       # rows the sdf term must skip: 0, 0.5, 2, -1
        "valid_odd": ~is_valid & (v != 0),
        "sign_out": ~is_free,                         # rows the free-space term must skip: 0, -1, 2, 0.5
        "sign_odd": ~is_free & (f != 0),
    }


PLANT_CYCLE = 8          # planted rows cycle through seven classes and one free draw
PLANT_ROWS = 64          # rows per class in a batch of at least PLANT_CYCLE * PLANT_ROWS rows


def planted_per_class(n):
    """Rows every planted class holds at least, in a batch of n rows."""
    return min(PLANT_ROWS, n // PLANT_CYCLE)


# --------------------------------------------------------------------------- lattice batches
def lattice(n, loss_type, seed=0):
    """A label batch on a dyadic lattice: pred, target in [-1, 1) and weight in (0, 1] are multiples of q = 2^-6 (L1) or
    2^-4 (L2), trunc = 0.25.  Every fp32 subtraction of the rule is exact on it and a tie is a tie in any precision.
    The first rows (then shuffled) are planted, class by class:
      valid rows with d == 0 | free rows with up == lo > 0 (s = (t + trunc) / 2, t < trunc) | free rows with
      up == lo == 0 | up > lo | lo > up | valid in {0, 0.5, 2, -1} on rows with d != 0 | sign in {0, -1, 2, 0.5} on
      rows with up > lo.
    -> dict(pred, target, valid, sign, weight: fp32 (n,), trunc, q, masks = classify(...))."""
    rs = np.random.RandomState(1000 + seed + (7 if loss_type == "L2" else 0))
    bits = 6 if loss_type == "L1" else 4
    q, R = 2.0 ** -bits, 2 ** bits                     # values k q with k in [-R, R)
    T = R // 4                                         # trunc = 0.25 in lattice units
    si, ti = rs.randint(-R, R, n), rs.randint(-R, R, n)
    wi = rs.randint(1, R + 1, n)
    valid = (rs.uniform(0, 1, n) > 0.1).astype(F32)
    sign = (rs.uniform(0, 1, n) > 0.5).astype(F32)
    for i in range(min(n, PLANT_CYCLE * PLANT_ROWS)):
        c, k = i % PLANT_CYCLE, i // PLANT_CYCLE
        if c == 0:
            valid[i], ti[i] = 1, si[i]
        elif c == 1:                                   # up = s - t = m, lo = trunc - s = m
            m = 1 + k % ((R + T) // 2)
            sign[i], si[i], ti[i] = 1, T - m, T - 2 * m
        elif c == 2:                                   # s >= trunc, t >= s
            sign[i], si[i] = 1, T + k % (R - T)
            ti[i] = si[i] + (k // 3) % (R - si[i])
        elif c == 3:                                   # s >= trunc (lo = 0), t < s
            sign[i], si[i] = 1, T + k % (R - T)
            ti[i] = si[i] - 1 - k % 5
        elif c == 4:                                   # s < trunc (lo > 0), t >= s (up = 0)
            sign[i], si[i] = 1, T - 1 - k % (R + T)
            ti[i] = min(R - 1, si[i] + k % 4)
        elif c == 5:
            valid[i] = (0.0, 0.5, 2.0, -1.0)[k % 4]
            ti[i] = si[i] - 1 if si[i] > -R else si[i] + 1
        elif c == 6:
            sign[i] = (0.0, -1.0, 2.0, 0.5)[k % 4]
            si[i] = T + k % (R - T)
            ti[i] = si[i] - 1 - k % 5
    p = rs.permutation(n)
    out = dict(pred=(si * q).astype(F32)[p], target=(ti * q).astype(F32)[p], valid=valid[p], sign=sign[p],
               weight=(wi * q).astype(F32)[p], trunc=T * q, q=q)
    assert np.all(np.abs(out["pred"]) <= 1) and np.all(np.abs(out["target"]) <= 1)
    out["masks"] = classify(out["pred"], out["target"], out["valid"], out["sign"], out["trunc"])
    return out


def assert_planted(batch, classes=("d0", "tie_pos", "tie_zero", "up_gt", "lo_gt", "valid_out", "sign_out"), odd=True):
    """Every planted class holds its rows (three of four outside-valued labels are not 0)."""
    n = len(batch["pred"])
    need = planted_per_class(n)
    counts = {k: int(m.sum()) for k, m in batch["masks"].items()}
    for c in classes:
        assert counts[c] >= need, (c, counts, need)
    if odd:
        for c in ("valid_odd", "sign_odd"):
            assert counts[c] >= (3 * need) // 4, (c, counts, need)
    return counts


# --------------------------------------------------------------------------- fp32 ties of the free-space maximum
def fs_ties(s, trunc):
    """Targets that put a prediction's free-space maximum ON its tie, from the prediction's own fp32 bits:
    lo = fl(trunc - s), t = fl(s - lo); the row is `kept` where lo > 0 and fl(s - t) == lo (up == lo > 0 on the device
    as here: single fp32 operations).  `strict` rows are kept rows whose tie both one-ulp neighbours of t break, the
    upper one towards lo > up and the lower one towards up > lo (a target much smaller than lo moves s - t by less than
    half an ulp of lo and leaves the tie in place: such rows are kept but not strict).
    -> t, t_up, t_down (fp32), kept, strict."""
    s = np.asarray(s, dtype=F32).reshape(-1)
    tr = F32(trunc)
    with np.errstate(invalid="ignore", over="ignore"):
        lo = tr - s
        t = s - lo
        kept = (lo > 0) & ((s - t) == lo) & np.isfinite(t)
        t_up, t_down = np.nextafter(t, F32(np.inf)), np.nextafter(t, F32(-np.inf))
        strict = kept & (np.maximum(s - t_up, F32(0)) < lo) & (np.maximum(s - t_down, F32(0)) > lo)
    return t, t_up, t_down, kept, strict


def planted_random(n, loss_type, seed=0):
    """An off-lattice batch: 0.2 randn predictions, labels as golden_cases.make_targets draws them, trunc = 0.15, and
    planted in the first rows (then shuffled): target == pred on valid rows; the fp32 tie of fs_ties on free rows (two
    rows of the cycle); its one-ulp neighbours above and below."""
    import golden_cases as gc
    rs = np.random.RandomState(2000 + seed + (7 if loss_type == "L2" else 0))
    s = (0.2 * rs.standard_normal(n)).astype(F32)
    t, valid, sign, weight = [a.reshape(-1).copy() for a in gc.make_targets(gc.CASES["small"], n)]
    trunc = 0.15
    tie, tie_up, tie_down, kept, _ = fs_ties(s, trunc)
    for i in range(min(n, PLANT_CYCLE * 2 * PLANT_ROWS)):
        c = i % PLANT_CYCLE
        if c == 0:
            valid[i], t[i] = 1, s[i]
        elif c in (1, 2) and kept[i]:
            sign[i], t[i] = 1, tie[i]
        elif c == 3 and kept[i]:
            sign[i], t[i] = 1, tie_up[i]
        elif c == 4 and kept[i]:
            sign[i], t[i] = 1, tie_down[i]
    p = rs.permutation(n)
    out = dict(pred=s[p], target=t[p], valid=valid[p], sign=sign[p], weight=weight[p], trunc=trunc)
    out["masks"] = classify(out["pred"], out["target"], out["valid"], out["sign"], out["trunc"])
    return out


# --------------------------------------------------------------------------- the launches and their rounding bounds
def column_launch(n, vec):
    """launch_mapping_loss (csrc/loss.hip): 256 threads, at most 64 blocks, grid-stride over n / 4 float4 items (all
    seven arrays 16-B aligned and n % 4 == 0) or n scalars.  -> (K, B): terms a thread adds in sequence, blocks."""
    items = n // 4 if vec else n
    blocks = min(64, (items + 255) // 256)
    per_thread = (items + blocks * 256 - 1) // (blocks * 256)
    return (4 if vec else 1) * per_thread, blocks


def takes_float4(n):
    return n % 4 == 0


def term_bounds(abs_sums, n, K, B, weights=(W_SDF, W_FS), div=None, lds_adds=2):
    """Rounding bound of the two loss terms as a kernel sums them:
        (K + 6 + lds_adds + B + 3) U  sum_i |term_i|  w / n
    K additions in a thread, 6 shuffle steps, lds_adds additions of the wavefronts' sums, B partial results added by
    atomics (0 where the test adds the per-workgroup slots itself, in float64), and 3 roundings of the scale: fl(1/fl(n)),
    w * sum, * inv_n.  Every addition is charged U times the WHOLE sum of magnitudes although all but the last B +
    lds_adds of them act on one wavefront's share of it; that slack also covers the (at most 3) roundings that form one
    term off the lattice."""
    div = float(n if div is None else div)
    return np.array([(K + 6 + lds_adds + B + 3) * U * a * w / div for a, w in zip(abs_sums, weights)])


def exact_sum_bounds(terms, B):
    """Where every partial sum is representable (see test_mapping_loss.py) the sums themselves are exact; what is left is
    fl(1/fl(n)), the product with it (w * sum is exact, w a power of two) and B atomic additions: (B + 2) roundings,
    none at all when n is a power of two and B == 1."""
    return gamma(B + 2) * np.abs(terms)


def fused_K(n):
    """Points one lane of sdf_fwd_kernel / sdf_train_kernel adds in sequence, at most: trips of 64 (or 32) points are
    dealt to eight groups of workgroups (ChunkSched, csrc/sdf_fused.hpp: ceil(trips / 8) consecutive trips per group)
    and inside a group to at least four wavefronts in turn.  Valid for launches of eight workgroups or more
    (n >= 2048: four wavefronts a workgroup, 64 points a trip)."""
    assert n >= 2048
    trips = (n + 31) // 32
    per_group = (trips + 7) // 8
    return (per_group + 3) // 4
