"""Inputs and bars of the tracker's device steps (tests/test_tracker_oracle.py on the CPU, tests/test_tracker_steps_oracle.py
on the GPU): a steep field, two geometries, label layouts, and the yardsticks both modules judge with.  Nothing here
touches the library; everything is generated from seeds.

The field is CASES["small"] (two levels, C = 4, hidden 32: fused-path eligible) with its features times 100: the
median |d sdf / dx| is then about 0.5 instead of 0.004, the diagonal of J^T J / n about 0.2, and H = J^T J dominates
the damping at every n >= 64 -- the normal equations, their unpacking and the pivoted solve all matter."""
import functools
import math

import numpy as np
import torch

import golden_cases as gc
from oracle import ref_torch as R

F32, F64 = torch.float32, torch.float64
CASE = gc.CASES["small"]
FEATURE_SCALE = 100.0
SIZES = (1, 63, 64, 65, 257, 33025)          # 33025 = 128 * 256 + 257: a second grid-stride trip for part of the grid
DR2 = (0.0, 1e-6, 2.5e-5, 4e-4, 0.09, 2.25)  # |dr|^2 of tests/test_pose_jacobian_oracle.py: >= 4x either side of the clamp
TRUNC = 0.25                                 # 50-90 % of the steep targets lie inside (asserted on the CPU)
GM_SCALE = 0.1
LAMBDA = {"steep": 0.5, "near_origin": 1e-4, "faces": 0.5}
KF = 1                                       # the keyframe id the rows carry
EPS32 = 2.0 ** -23
COND_MAX = 1e4                               # the solve bar's premise: cond_inf(H + lambda I) of the case, from the oracle

# ---- bars (each derived where it is used; the CPU module proves they reject real faults) ------------------------------
POSE_BAR = 4 * EPS32                # about 8 fp32 operations per pose entry; |R_ij| <= 1, t relative
SDF_REL = 2e-6                      # tests/test_split_precision.py: 2e-6 max(1, |sdf|max)
SUMS_REL = 1e-5                     # pair_sums_excess's: <= 2 fp32 adds per thread, fp64 fan-in, <= 128 fp32 atomics
GPRED_REL = 4 * EPS32               # per row: subtract, (weight), multiply by 2, by weight, by 1/n
LOSS_REL = 1e-6
PULL_REL = 1e-6                     # of the absolute-value pull-back (tests/test_pose_jacobian_oracle.py, epilogue A)
MOMENT_RTOL = 2e-6                  # m, v (ibid., epilogue B)
NORM_REL = 1e-5                     # info[0:3]


# seeds per (geometry, n) of the LM cases: chosen so that at least one row is kept (n = 1) and, near the origin, the
# fp64 LU of H + lambda I exchanges rows (tests/test_tracker_oracle.py asserts both)
LM_SEEDS = {"steep": {1: 1, 63: 0, 64: 0, 65: 0, 257: 0, 33025: 0}, "near_origin": {1: 0, 64: 0, 257: 0}}


def pose_ratio(got, want):
    """worst |got - want| / bar over the 12 pose entries, the bar being POSE_BAR absolute for R (entries <= 1) and
    POSE_BAR |t| for t; <= 1 passes, NaN counts as inf"""
    got, want = (torch.as_tensor(t, dtype=F64).detach().cpu().reshape(12) for t in (got, want))
    bar = POSE_BAR * torch.cat([torch.ones(9, dtype=F64), want[9:].abs()])
    r = ((got - want).abs() / bar.clamp_min(1e-300)).max()
    return float("inf") if torch.isnan(r) else float(r)


def param_atol(lr):
    return 1e-7 + 1e-6 * lr


def sums_excess(got, sums, A, exact=()):
    """how far each kernel sum lies beyond SUMS_REL A + 1e-12 (positive: a failure; NaN counts as one); the entries
    of ``exact`` must be equal"""
    got, sums, A = (torch.as_tensor(t, dtype=F64).detach().cpu().reshape(-1) for t in (got, sums, A))
    ex = (got - sums).abs() - (SUMS_REL * A + 1e-12)
    for i in exact:
        ex[i] = -1.0 if got[i] == sums[i] else max(abs(float(got[i] - sums[i])), 1.0)
    return torch.where(torch.isnan(ex), torch.full_like(ex, float("inf")), ex)


def solve_bar(sums, lam):
    """(fp64 delta, cond_inf, bar on |delta_kernel - delta|_inf): 8 x the error of fp32 torch.linalg.solve on the CPU
    for the same system -- the reference's own arithmetic --, taken no smaller than 8 x the half ulp (2^-24 |delta|_inf)
    that the rounding of any fp32 result to its own format costs: one realisation that happens to land closer says
    nothing about another solver's.  Where cond_inf > COND_MAX the sample is noise (measured: the kernel's own
    algorithm restated in numpy lands at 0.5 .. 9 x of it at cond 2e4 .. 1.4e5), and the bar is the forward bound of a
    backward-stable solve instead, cond_inf 2^-24 |delta|_inf."""
    delta, cond = R.lm_solve64(sums, lam)
    H, g = R.lm_unpack(sums)
    d32 = torch.linalg.solve((H + lam * torch.eye(6, dtype=F64)).float(), -g.float()).double()
    scale = delta.abs().max().item()
    bar = max(8.0 * (d32 - delta).abs().max().item(), 4 * EPS32 * scale, 1e-30)
    if cond > COND_MAX:
        bar = max(bar, cond * 0.5 * EPS32 * scale)
    return delta, cond, bar


def solve32(sums, lam, wrong_slot=False, skip_swap=False, swap_without_rhs=False):
    """lm_solve_kernel restated in numpy fp32, step by step (unpack, damp, LU with partial pivoting on the augmented
    matrix, back substitution) -> delta (6,) fp64.  wrong_slot: H[0][3] and H[3][0] read from the slot of H[0][4];
    skip_swap: the pivot search runs but the rows stay where they are; swap_without_rhs: the exchange leaves column 6
    (the right-hand side) behind."""
    s = np.asarray(torch.as_tensor(sums, dtype=F64).detach().cpu().reshape(-1).numpy(), dtype=np.float32)
    f = np.float32
    A = np.zeros((6, 7), dtype=np.float32)
    o = 0
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = s[o]
            o += 1
    if wrong_slot:
        A[0, 3] = A[3, 0] = s[4]
    for a in range(6):
        A[a, a] = f(A[a, a] + f(lam))
        A[a, 6] = -s[21 + a]
    for c in range(6):
        p = c
        for r in range(c + 1, 6):
            if abs(A[r, c]) > abs(A[p, c]):
                p = r
        if p != c and not skip_swap:
            m = 6 if swap_without_rhs else 7
            A[[c, p], :m] = A[[p, c], :m]
        inv = f(1.0) / A[c, c]
        for r in range(c + 1, 6):
            fac = f(A[r, c] * inv)
            for j in range(c, 7):
                A[r, j] = f(A[r, j] - f(fac * A[c, j]))
    d = np.zeros(6, dtype=np.float32)
    for r in range(5, -1, -1):
        v = A[r, 6]
        for j in range(r + 1, 6):
            v = f(v - f(A[r, j] * d[j]))
        d[r] = f(v / A[r, r])
    return torch.from_numpy(d.astype(np.float64))


# ---- the field -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def field():
    """{feats [(1,C,Z,Y,X) fp32], bound (3,2) fp32, ws, bs}: CASES["small"], features times FEATURE_SCALE"""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    feats = [T(f) * FEATURE_SCALE for f in gc.make_features(CASE)]
    ws, bs = R.decoder_params({k: T(v) for k, v in gc.make_decoder(CASE).items()})
    return dict(feats=feats, bound=torch.tensor(CASE["bound"], dtype=F32), ws=ws, bs=bs)


def field_eval(xw, dtype=F64):
    """SDF (n,), its spatial gradient (n,3) and the smallest |ReLU pre-activation| (n,) at points ``xw`` (fp32 from a kernel, or fp64), in
    ``dtype``: encode_gather + the decoder chain + autograd.  A row with a non-finite coordinate is evaluated at the
    origin instead: safe_rows never calls it safe."""
    fl = field()
    x = torch.as_tensor(xw).detach().cpu().to(dtype)
    x = torch.where(torch.isfinite(x).all(1, keepdim=True), x, torch.zeros_like(x)).requires_grad_(True)
    h = R.encode_gather([f.to(dtype) for f in fl["feats"]], fl["bound"].to(dtype), x)
    premin = torch.full((x.shape[0],), float("inf"), dtype=dtype)
    last = len(fl["ws"]) - 1
    for i, (w, b) in enumerate(zip(fl["ws"], fl["bs"])):
        h = torch.nn.functional.linear(h, w.to(dtype), b.to(dtype))
        if i != last:
            premin = torch.minimum(premin, h.detach().abs().min(dim=1).values)
            h = torch.relu(h)
    (g,) = torch.autograd.grad(h.sum(), x)
    return h.detach()[:, 0], g, premin


def safe_rows(xw, premin):
    """(n,) bool: >= 1e-3 index units from every cell plane of every level (fd_safe), >= 1e-4 m from every face of the
    bound, >= 1e-4 in every ReLU pre-activation -- where the field and its gradient are smooth, so that an fp32
    evaluation and the fp64 one are on the same piece."""
    fl = field()
    x = torch.as_tensor(xw).detach().cpu().double()
    b = fl["bound"].double()
    ok = torch.isfinite(x).all(1) & (premin >= 1e-4)
    xn = R.normalize_coordinates(torch.nan_to_num(x), b)
    for f in fl["feats"]:
        ok &= R.fd_safe(xn, (f.shape[4], f.shape[3], f.shape[2]), False)
    for a in range(3):
        ok &= ((x[:, a] - b[a, 0]).abs() >= 1e-4) & ((x[:, a] - b[a, 1]).abs() >= 1e-4)
    return ok


# ---- geometries ------------------------------------------------------------------------------------------------------
def correction(dr2, seed):
    """(dr (3,), dt (3,)) fp32: a rotation correction of squared length dr2 in a random direction, a small translation"""
    rs = np.random.RandomState(1000 + seed)
    d = rs.standard_normal(3)
    dr = torch.tensor(d / np.linalg.norm(d) * math.sqrt(dr2), dtype=F32)
    return dr, torch.tensor(rs.uniform(-0.02, 0.02, 3), dtype=F32)


def geometry(kind, n, seed=0):
    """One keyframe batch: {x (n,3) fp32 samples in the keyframe frame, R_base (3,3), t_base (3,), target (n,) fp32,
    lm_lambda, trunc}.

    steep: x uniform in a box of the bound's size around the frame origin, R_base = rodrigues(+-0.3), t_base the
      bound's centre plus an offset, so that most but not all rows land inside; target = oracle SDF at the base pose
      times (1 + 0.5 u), so |target| straddles TRUNC.
    near_origin: |x|_inf <= 0.02 m, t_base mid-bound, lm_lambda 1e-4: the rotation block of H is ~|x|^-2 smaller than
      the translation block, column 0's largest entry is off the diagonal and the LU swaps rows.
    faces: identity R_base, dyadic t_base and x such that the mapped samples are face_rows(n): a 1/64 m lattice with
      a handful of rows exactly on the faces of FACE_BOUND (the count is inclusive); targets 0."""
    g = torch.Generator().manual_seed(77 + 1000 * seed + n)
    rs = np.random.RandomState(seed + 5)
    b = field()["bound"].double()
    centre, half = (b[:, 0] + b[:, 1]) / 2, (b[:, 1] - b[:, 0]) / 2
    u = torch.rand(n, generator=g, dtype=F64)
    if kind == "steep":
        x = ((torch.rand(n, 3, generator=g, dtype=F64) * 2 - 1) * half).float()
        R_base = torch.tensor(gc.rodrigues(rs.uniform(-0.3, 0.3, 3)), dtype=F32)
        t_base = (centre + torch.tensor([0.15, -0.1, 0.1], dtype=F64)).float()
    elif kind == "near_origin":
        x = ((torch.rand(n, 3, generator=g, dtype=F64) * 2 - 1) * 0.02).float()
        R_base = torch.tensor(gc.rodrigues(rs.uniform(-0.3, 0.3, 3)), dtype=F32)
        t_base = centre.float()
    elif kind == "faces":
        R_base = torch.eye(3, dtype=F32)
        t_base = torch.tensor([0.25, -0.125, 1.0], dtype=F32)
        return dict(x=(face_rows(n) - t_base.double()).float(), R_base=R_base, t_base=t_base, lm_lambda=LAMBDA[kind],
                    trunc=TRUNC, target=torch.zeros(n))
    else:
        raise ValueError(kind)
    xw, _ = R.track_transform32(x, R.track_pose64(R_base, t_base, torch.zeros(3), torch.zeros(3)).float())
    sdf, _, _ = field_eval(xw)
    return dict(x=x, R_base=R_base, t_base=t_base, target=(sdf * (1 + 0.5 * u)).float(), lm_lambda=LAMBDA[kind],
                trunc=TRUNC)


FACE_BOUND = [[-1.0, 1.25], [-0.75, 0.875], [0.0, 2.125]]       # dyadic faces: the lattice reaches them exactly


def face_rows(n):
    """world points (n,3) fp64 on the 1/64 lattice with the first min(n, 12) rows on exact faces of FACE_BOUND: row i
    sits on the min (even i) or max (odd i) face of axis (i // 2) % 3, rows 6.. one lattice step outside it"""
    g = torch.Generator().manual_seed(4242 + n)
    b = torch.tensor(FACE_BOUND, dtype=F64)
    q = torch.stack([torch.randint(int(b[a, 0] * 64) + 1, int(b[a, 1] * 64), (n,), generator=g) for a in range(3)], 1).double() / 64
    for i in range(min(n, 12)):
        ax, side = (i // 2) % 3, i % 2
        q[i, ax] = b[ax, side] + (0.0 if i < 6 else (1.0 if side else -1.0) / 64)
    return q


# ---- label layouts ---------------------------------------------------------------------------------------------------
LAYOUTS = ("plain", "block_bool", "block_float", "sanitize", "no_filter")


def labels(layout, geo, seed=0, holes=False):
    """The batch's label columns as the tracker hands them over, on the CPU (the GPU module moves the block, then takes
    the same views): {target, valid, frame_ids, sanitize, trunc, x}.

    plain: contiguous (n,) target, no valid column, no frame ids, sanitize=False.
    block_bool: target = column 0 of an (n,4) block (stride 4), valid bool (n,1), frame_ids (n,1); ``holes``: ~10 % of the
      rows invalid (the Adam window masks them; the LM step counts them and leaves the pose alone).
    block_float: the same with valid = column 1 of the block, float, stride 4.
    sanitize: block_bool's columns, sanitize=True, a NaN and a +-inf among coordinates and targets.
    no_filter: plain with trunc None (every row kept)."""
    n = geo["x"].shape[0]
    g = torch.Generator().manual_seed(31 + seed + n)
    x, tgt = geo["x"].clone(), geo["target"].clone()
    out = dict(x=x, sanitize=False, trunc=geo["trunc"], valid=None, frame_ids=None)
    if layout in ("plain", "no_filter"):
        out["target"] = tgt
        if layout == "no_filter":
            out["trunc"] = None
        return out
    block = torch.stack([tgt, torch.ones(n), torch.zeros(n), torch.ones(n)], dim=1)
    if holes:
        block[:, 1] = (torch.rand(n, generator=g) > 0.1).float()
    if layout == "sanitize":
        out["sanitize"] = True
        # a NaN coordinate (-> 0: the row stays), a NaN target (-> 0: kept), +-inf targets (-> +-FLT_MAX: filtered),
        # and +-inf coordinates on rows whose target is filtered (their samples map to +-inf / NaN: nothing to sum)
        if n >= 8:
            x[2, 1] = float("nan")
            tgt_bad = {3: float("nan"), 4: float("inf"), 5: float("-inf"), 6: float("inf"), 7: float("-inf")}
            for i, v in tgt_bad.items():
                block[i, 0] = v
            x[6, 0] = float("inf")
            x[7, 2] = float("-inf")
        else:
            block[0, 0] = float("nan")
            x[0, 1] = float("nan")
    out["block"] = block
    out["target"] = block[:, 0:1]
    out["valid"] = block[:, 1:2] if layout == "block_float" else (block[:, 1:2] > 0)
    out["frame_ids"] = torch.full((n, 1), KF, dtype=torch.int64)
    return out


# ---- the kernels' own arithmetic restated (what the bars must accept), with switches for the faults they must reject ----
def pull_back_formula(R_base, dr, sums, no_transpose=False, drop_dadb=False):
    """track_adam_kernel + so3_exp_backward (align.hpp) restated in numpy fp64, term by term: G = R_base^T gR,
    d/dw = a vee(G - G^T) + b vee(M - M^T) + (a'/th <G,K> + b'/th <G,K^2>) w with M = G K^T + K^T G; the last term only
    where |w|^2 >= 1e-4.  -> g6 (6,) fp64.  no_transpose: G = R_base gR; drop_dadb: without the a', b' term."""
    s = torch.as_tensor(sums, dtype=F64).detach().cpu().reshape(-1).numpy()
    Rb = torch.as_tensor(R_base, dtype=F64).detach().cpu().reshape(3, 3).numpy()
    w32 = torch.as_tensor(dr, dtype=F32).detach().cpu().reshape(3).numpy()
    w = w32.astype(np.float64)
    G = (Rb if no_transpose else Rb.T) @ s[:9].reshape(3, 3)
    sq = float(np.float32(np.float32(np.float32(w32[0] * w32[0]) + np.float32(w32[1] * w32[1])) + np.float32(w32[2] * w32[2])))
    live = sq >= float(np.float32(1e-4)) and not drop_dadb
    th = math.sqrt(max(sq, 1e-4))
    sn, cs = math.sin(th), math.cos(th)
    a, b = sn / th, (1.0 - cs) / (th * th)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    M = G @ K.T + K.T @ G
    da = (th * cs - sn) / (th * th) / th if live else 0.0
    db = (th * sn - 2.0 * (1.0 - cs)) / (th ** 3) / th if live else 0.0
    vee = lambda X: np.array([X[2, 1] - X[1, 2], X[0, 2] - X[2, 0], X[1, 0] - X[0, 1]])
    gw = a * vee(G) + b * vee(M) + (da * (G * K).sum() + db * (G * (K @ K)).sum()) * w
    return torch.from_numpy(np.concatenate([gw, s[9:12]]))


def adam32(param, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8):
    """adam_one (common.hpp) with the step scalars of miso_adam_scalars_table, in numpy fp32 -> (param, m, v) fp64"""
    f = np.float32
    c = lambda z: np.asarray(torch.as_tensor(z, dtype=F64).detach().cpu().reshape(-1).numpy(), dtype=f)
    p, g, m, v = c(param), c(g), c(m), c(v)
    b1, b2 = betas
    omb1, b2f, omb2 = f(1 - b1), f(b2), f(1 - b2)
    nss, bc2s, epsf = f(-lr / (1 - b1 ** t)), f(math.sqrt(1 - b2 ** t)), f(eps)
    m = m + omb1 * (g - m)
    v = v * b2f + (omb2 * g) * g
    p = p + (nss * m) / (np.sqrt(v) / bc2s + epsf)
    return tuple(torch.from_numpy(z.astype(np.float64)) for z in (p, m, v))


def gpred32(sdf, gt, ok, n, loss_type, weight, gm_scale=GM_SCALE, gm_unsquared=False, mean_over_kept=False):
    """track_loss_kernel's per-row line in torch fp32, operation by operation -> (loss fp64, gpred (n,) fp64).
    gm_unsquared: w = c / (c + r^2); mean_over_kept: 1 / (rows of ``ok``) for 1 / n."""
    sdf, gt = (torch.as_tensor(t).detach().cpu().to(F32).reshape(-1) for t in (sdf, gt))
    ok = torch.as_tensor(ok).detach().cpu().reshape(-1).bool()
    one, wgt = torch.tensor(1.0, dtype=F32), torch.tensor(float(weight), dtype=F32)
    inv_n = one / torch.tensor(float(int(ok.sum()) if mean_over_kept else n), dtype=F32)
    r = torch.where(ok, sdf - gt, torch.zeros_like(sdf))
    if loss_type == "L2":
        term, d = r * r, 2 * r
    elif loss_type == "L1":
        term, d = r.abs(), torch.sign(r)
    else:
        c = torch.tensor(float(gm_scale), dtype=F32)
        q = c + r * r
        w = c / q if gm_unsquared else c / (q * q)
        term, d = w * r * r, w * 2 * r
    every = torch.ones_like(ok)
    part = R._kernel_fan_in(term[:, None], every, F64)[0]
    return float(part) * float(wgt) * float(inv_n), torch.where(ok, wgt * d * inv_n, torch.zeros_like(d)).double()
