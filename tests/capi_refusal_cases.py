"""The refusals of the C ABI layer (miso_amd/csrc/capi.hip) as a table: one recipe of a valid call per entry point, and
from it the single-fault cases -- exactly one argument or struct field changed -- that the layer must refuse before any
HIP call.  The library loads without a GPU and every refusal is host code, so the whole table is recorded and replayed
on a machine without one.

  python tests/capi_refusal_cases.py --record     writes tests/golden/capi_refusals.json (name -> code or value)
  (MISO_HIP_LIB=<path of another build's libmiso_hip.so> in front records from that build)

The recorded file is the contract: record it from a build of the commit whose behaviour is to be kept (the parent of a
refactor; the head after a deliberate behaviour change, with the diff of the JSON in the review), then
tests/test_capi_refusals.py replays the cases against the library of the tree and compares.

Rules the cases follow:
  * the valid call of a LAUNCHING entry point is never issued, nor any case that would reach a launcher: every case of
    such an entry point must come back 2001, 2002 or 2003 -- the recorder aborts otherwise, and the case is then no
    refusal and does not belong here.  Whether an argument is optional is read off miso_hip.h and capi.hip.
  * pointers are addresses inside one live, 16-byte-aligned host buffer (never read by a refusal); host arrays that an
    entry point does read (bounds, strides, plans) are real ctypes arrays.
  * the pure host queries (HOST below) also record the valid call: its value, or the bytes of the struct it writes.

Every `return MISO_E_*` statement of capi.hip is reached by a case (checked once with a counter per statement in a
scratch build), where need be through a second recipe of the entry point (the "/variant" names), except one:
  * miso_nn_plan, `if (!(c < inf)) return MISO_E_BADARG` inside the loop that doubles the cell: the extents are finite
    by then, so the cell count has fallen to <= 27 while the doubled cell is still finite.  No input reaches it.
"""
import ctypes as C
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "capi_refusals.json")
REFUSALS = (2001, 2002, 2003)
INF = float("inf")

from miso_amd import _lib  # noqa: E402

# ---- live memory ------------------------------------------------------------------------------------------------------
_ARENA = C.create_string_buffer(1 << 20)
_BASE = (C.addressof(_ARENA) + 255) & ~255
_next = [0]


def P(nbytes=256):
    """a fresh address in the arena, 256-byte aligned"""
    a = _BASE + _next[0]
    _next[0] += (nbytes + 255) & ~255
    assert _next[0] < (1 << 20) - 256
    return a


def floats(*v):
    arr = (C.c_float * len(v))(*v)
    _KEEP.append(arr)
    return C.addressof(arr)


def int64s(*v):
    arr = (C.c_int64 * len(v))(*v)
    _KEEP.append(arr)
    return C.addressof(arr)


_KEEP = []
LO, HI = floats(0, 0, 0), floats(1, 1, 1)

# ---- valid structs, filled as _lib's callers fill them -------------------------------------------------------------------
N = 5            # points of a recipe
F = 8            # features of the recipe grid: 2 levels x 4 channels
TILES_XYZ = 2 | (2 << 8) | (2 << 16)       # MISO_TILES_XYZ(2, 2, 2): a per-axis binning
ROWS_2GB = 1 << 26                         # n at which n * F * 4 bytes reach 2 GB


def grid(grad=False, flags=0):
    """2 levels of (1, 4, 3, 3, 3), channels last; the levels behind n_levels are filled alike, so that a case which
    only raises n_levels meets valid levels"""
    g = _lib.Grid()
    g.n_levels, g.ignore_mask, g.flags = 2, 0, flags
    for a in range(3):
        g.bound_min[a], g.bound_max[a] = 0.0, 1.0
    for l in range(_lib.MAX_LEVELS):
        s = g.level[l]
        s.data = P(512)
        s.grad = P(512) if grad and l < 2 else None
        s.C, s.X, s.Y, s.Z = 4, 3, 3, 3
        s.sC, s.sX, s.sY, s.sZ = 1, 4, 12, 36
    return g


def mlp():
    m = _lib.Mlp()
    m.in_dim, m.hidden_dim, m.out_dim, m.n_linear = F, 64, 1, 3
    for i in range(3):
        m.weight[i] = P(64 * 64 * 4)
    return m


def mlp_grad():
    g = _lib.MlpGrad()
    for i in range(3):
        g.weight[i] = P(64 * 64 * 4)
    return g


def binned(tiles=2):
    s = _lib.Sorted()
    s.tiles_per_axis = tiles
    s.x_sorted, s.xn_sorted, s.perm, s.tile_offsets = None, P(), P(), P()
    return s


def nn_plan():
    p = _lib.NnPlan()
    p.cell, p.coord_mag, p.max_rings, p.n_tgt, p.cells = 0.5, 3.0, 8, 10, 27
    for a in range(3):
        p.dims[a] = 3
    return p


def mesh_plan(cell=0.5):
    p = _lib.MeshPlan()
    p.cell, p.coord_mag, p.widen, p.n_tri, p.cells = cell, 3.0, 3.0 * 2.0 ** -17, 4, 27
    for a in range(3):
        p.dims[a] = 3
    return p


def lm_track():
    a = _lib.LmTrack()
    a.coords_frame, a.target, a.valid, a.frame_ids = P(), P(), P(), P()
    a.stride_target = a.stride_valid = a.stride_frame_ids = 1
    a.n, a.keyframe_id, a.trunc_dist = N, 0, 0.1
    a.R_base, a.t_base, a.rot_correction, a.trans_correction = P(), P(), P(), P()
    a.loss_type, a.gm_scale, a.lm_lambda = 2, 1.0, 1e-3
    a.pose, a.coords_world, a.sdf, a.grad, a.ones, a.relu_mask, a.sums, a.info = P(), P(), P(), P(), P(), P(4096), P(), P()
    return a


def track_adam():
    t = _lib.TrackAdam()
    t.s = lm_track()
    t.loss_type, t.weight_sdf, t.gm_scale = 2, 1.0, 1.0
    t.grad_pred, t.adam_table, t.adam_table_len, t.state, t.loss_ring, t.ring_len = P(), P(), 4, P(), P(), 4
    return t


def adam_tensor():
    t = _lib.AdamTensor()
    t.param, t.grad, t.exp_avg, t.exp_avg_sq, t.active, t.touched = P(), P(), P(), P(), P(), P()
    t.numel, t.zero_grad = 8, 1
    return t


def adam_when(device=False):
    w = _lib.AdamWhen()
    w.lr, w.beta1, w.beta2, w.eps, w.step, w.table_len = 1e-3, 0.9, 0.999, 1e-8, 1, 4      # (host form: table_len unread)
    if device:
        w.step, w.table, w.step_dev = 0, P(), P()
    return w


def align_pair(lattice=False):
    p = _lib.AlignPair()
    p.dst_grid = grid()
    p.coords_src, p.feats_src, p.ld_feats, p.n = P(), P(), F, N
    p.gate_n, p.src, p.dst = 4, 0, 1
    if lattice:
        for a in range(3):
            p.gate_axis[a] = P()
            p.gate_dims[a] = (2, 2, 1)[a]
    else:
        p.gate_coords = P()
    return p


def align_cfg(iterating=False):
    c = _lib.Align()
    c.n_submaps, c.n_pairs, c.loss_type, c.ring_iters = 2, 1, 2, 4
    c.lr, c.beta1, c.beta2, c.eps = 1e-3, 0.9, 0.999, 1e-8
    if iterating:
        c.R0, c.t0, c.plan, c.state = P(), P(), P(), P()
    return c


def ray_frames():
    f = _lib.RayFrames()
    f.depth, f.T_WC, f.R_wk, f.t_wk = P(), P(), P(), P()
    f.n_frames, f.H, f.W = 1, 4, 4
    f.fx = f.fy = f.cx = f.cy = 2.0
    return f


def ray_sampling():
    c = _lib.RaySampling()
    c.min_depth, c.dist_behind_surf, c.trunc_dist = 0.1, 0.1, 0.1
    c.n_strat, c.n_surf, c.rays_per_frame = 2, 2, 4
    return c


# ---- faults: (label, argument, new value | function of the old value) --------------------------------------------------------
def _fmt(v):
    if v is None:
        return "NULL"
    if isinstance(v, int) and abs(v) >= 1 << 20:
        for e in range(20, 64):
            if v == 1 << e:
                return f"2^{e}"
            if v == (1 << e) + 1:
                return f"2^{e}+1"
        return "given"                                 # an address: not part of a stable name
    return repr(v)


def null(*names):
    return [(f"{n}=NULL", n, None) for n in names]


def off(by, *names):
    """the pointer moved off its alignment rule by the smallest amount that breaks it"""
    return [(f"{n}+{by}", n, lambda v, by=by: v + by) for n in names]


def val(name, *values):
    return [(f"{name}={_fmt(v)}", name, v) for v in values]


def _walk(obj, path):
    tokens = re.findall(r"\[(\d+)\]|(\w+)", path)
    for idx, field in tokens[:-1]:
        obj = obj[int(idx)] if idx else getattr(obj, field)
    return obj, tokens[-1]


def _get(obj, path):
    obj, (idx, field) = _walk(obj, path)
    return obj[int(idx)] if idx else getattr(obj, field)


def _set(obj, path, v):
    obj, (idx, field) = _walk(obj, path)
    if idx:
        obj[int(idx)] = v
    else:
        setattr(obj, field, v)


def _clone(s):
    return type(s).from_buffer_copy(s)


def fld(name, path, *values):
    """one field of a struct argument (a copy of the recipe's) set to a value that breaks its rule"""
    def edit(v):
        return lambda s: (lambda c: (_set(c, path, v), c)[1])(_clone(s))
    sep = "" if path.startswith("[") else "."
    return [(f"{name}{sep}{path}={_fmt(v)}", name, edit(v)) for v in values]


def fld_off(by, name, *paths):
    def edit(path):
        return lambda s: (lambda c: (_set(c, path, _get(c, path) + by), c)[1])(_clone(s))
    return [(f"{name}.{p}+{by}", name, edit(p)) for p in paths]


def grid_faults(name, need_data, pre=""):
    """every rule of convert_grid (pre: the path of a grid nested in a struct argument)"""
    f = fld(name, pre + "n_levels", 0, _lib.MAX_LEVELS + 1) + fld(name, pre + "flags", 1 << 20)
    f += fld(name, pre + "level[0].C", 0) + fld(name, pre + "level[1].X", 0) + fld(name, pre + "level[1].Y", 0)
    f += fld(name, pre + "level[0].Z", 0)
    f += fld(name, pre + "level[0].sC", -1) + fld(name, pre + "level[0].sX", -1) + fld(name, pre + "level[1].sY", -1)
    f += fld(name, pre + "level[1].sZ", -1, 1 << 30)          # 2 * 2^30 + ... : a span >= 2^31
    if need_data:
        f += fld(name, pre + "level[1].data", None)
    return f


def fused_faults(g, m, vec4=True):
    """every rule of fused_shape; vec4: the call needs 16-byte addressable, channels-last levels (the atlas calls take
    that from their plan, not from `shape`)"""
    f = null(m) + fld(m, "n_linear", 1, _lib.MAX_LINEAR + 1) + fld(m, "out_dim", 2) + fld(m, "in_dim", F + 4)
    f += fld(m, "hidden_dim", 48)                              # outside MISO_FUSED_SHAPES
    f += fld(g, "level[1].C", 8)                               # channel counts differ between the levels
    f += fld(g, "n_levels", 5)                                 # (4, 5, 64, 1) is not in MISO_FUSED_SHAPES (in_dim != F first)
    if vec4:
        f += fld(g, "level[0].sX", 5) + fld(g, "level[1].sC", 2) + fld_off(4, g, "level[0].data")
    return f


def sorted_faults(name, perm_optional=False):
    f = null(name) + fld(name, "tile_offsets", None) + fld(name, "xn_sorted", None) + fld_off(4, name, "xn_sorted")
    f += fld(name, "tiles_per_axis", 0, 17, 255, 33 | (1 << 8) | (1 << 16), 1 << 24)
    if not perm_optional:
        f += fld(name, "perm", None)
    return f


def plan_faults(name, kind):
    mx = _lib.NN_MAX_CELLS
    f = null(name) + fld(name, "n_tgt" if kind == "nn" else "n_tri", -1, 1 << 31)
    f += fld(name, "dims[0]", 0) + fld(name, "dims[1]", 0) + fld(name, "dims[2]", 0)
    f += fld(name, "cells", 0, 28, mx + 1) + fld(name, "dims[0]", mx + 1)
    f += fld(name, "cell", 0.0, INF, float("nan")) + fld(name, "coord_mag", -1.0)
    if kind == "nn":
        f += fld(name, "max_rings", -1, _lib.NN_MAX_RINGS + 1)
    else:
        f += fld(name, "coord_mag", INF) + fld(name, "widen", -1.0, 4.0)
    return f


LOSS = dict(loss_type=1, weight_sdf=1.0, weight_fs=0.5, trunc_dist=0.1)
LOSS_FAULTS = val("loss_type", 0, 3)
BIG = 1 << 31

RECIPES = []      # (name, variant, args, faults, launches)
HOST = set()      # the entry points that never launch: their valid call is recorded too


def R(name, faults, variant="", host=False, **args):
    once = {}
    for f in faults:                                  # the fault lists of two families may name the same case
        once.setdefault(f[0], f)
    RECIPES.append((name, variant, args, list(once.values())))
    if host:
        HOST.add(name)


def build_recipes():
    g, gg, m, s = grid(), grid(grad=True), mlp(), binned()
    packed = P(1 << 16)
    PK = null("packed") + off(4, "packed")

    # ---- encode (every call that reads points has two recipes: "/x" the caller's order, "/sorted" a binned batch)
    enc_fwd = null("grid", "feats") + val("n", -1) + val("ld_out", F - 1) + grid_faults("grid", True)
    R("miso_encode_fwd", enc_fwd + null("x"), variant="x", grid=g, x=P(), sorted=None, n=N, feats=P(), ld_out=F,
      stream=None)
    R("miso_encode_fwd", enc_fwd + sorted_faults("sorted"), variant="sorted", grid=g, x=None, sorted=s, n=N, feats=P(),
      ld_out=F, stream=None)
    enc_bwd = null("grid", "grad_feats") + val("n", -1) + val("ld_g", F - 1) + grid_faults("grid", True)
    R("miso_encode_bwd", enc_bwd + null("x"), variant="x", grid=g, x=P(), sorted=None, n=N, grad_feats=P(), ld_g=F,
      grad_x=P(), stream=None)
    R("miso_encode_bwd", enc_bwd + sorted_faults("sorted"), variant="sorted", grid=g, x=None, sorted=s, n=N,
      grad_feats=P(), ld_g=F, grad_x=P(), stream=None)
    bwd2 = (null("grid", "grad_feats", "gg_out") + val("n", -1) + val("ld_g", F - 1) + val("ld_gg", F - 1) +
            grid_faults("grid", True) + fld("gg_grid", "n_levels", 1) + fld("gg_grid", "level[1].C", 8) +
            fld("gg_grid", "level[0].sZ", 40))
    R("miso_encode_bwd2", bwd2 + null("x"), variant="x", grid=g, gg_grid=grid(), x=P(), sorted=None, n=N, grad_feats=P(),
      ld_g=F, gg_x=P(), gg_out=P(), ld_gg=F, g_x=P(), stream=None)
    R("miso_encode_bwd2", bwd2 + sorted_faults("sorted"), variant="sorted", grid=g, gg_grid=grid(), x=None, sorted=s, n=N,
      grad_feats=P(), ld_g=F, gg_x=P(), gg_out=P(), ld_gg=F, g_x=P(), stream=None)

    # ---- decoder queries and packing
    mq = (null("mlp") + fld("mlp", "n_linear", 1, 5) + fld("mlp", "out_dim", 2) + fld("mlp", "in_dim", 0, 33) +
          fld("mlp", "hidden_dim", 48))
    R("miso_mlp_packed_floats", mq, host=True, mlp=m)
    R("miso_sdf_mask_words", null("mlp"), host=True, mlp=m)
    R("miso_mlp_pack", mq + null("packed") + fld("mlp", "weight[1]", None), mlp=m, packed=packed, stream=None)
    shape_q = null("grid") + grid_faults("grid", False) + fused_faults("grid", "mlp")
    R("miso_sdf_train_lds_bytes", shape_q, host=True, grid=g, mlp=m, scattering=0)
    R("miso_sdf_train_lds_bytes", [], variant="scattering", host=True, grid=g, mlp=m, scattering=1)
    R("miso_sdf_supported", shape_q, host=True, grid=g, mlp=m)
    R("miso_sdf_wgrad_workspace_floats", shape_q + val("n", -1), host=True, grid=g, mlp=m, n=N)
    R("miso_sdf_bwd_workspace_floats", null("grid") + grid_faults("grid", False) + val("n", -1), host=True, grid=g, n=N)

    # ---- fused forward / backward
    fused = null("grid") + grid_faults("grid", True) + fused_faults("grid", "mlp") + PK + val("n", -1)
    # (the "/x" recipes also hand over, one at a time, what belongs to the binned form: n_live, workspace, GRAD_SDF_SORTED)
    R("miso_sdf_fwd", fused + null("x", "sdf"), variant="x", grid=g, mlp=m, packed=packed, x=P(), sorted=None, n=N,
      sdf=P(), relu_mask=P(4096), stream=None)
    R("miso_sdf_fwd", fused + null("sdf") + sorted_faults("sorted"), variant="sorted", grid=g, mlp=m, packed=packed,
      x=None, sorted=s, n=N, sdf=P(), relu_mask=P(4096), stream=None)
    bwd = fused + null("grad_sdf", "relu_mask")
    R("miso_sdf_bwd", bwd + null("x") + val("workspace", P()) + fld("grid", "flags", 16), variant="x", grid=g, mlp=m,
      packed=packed, x=P(), sorted=None, n=N, grad_sdf=P(), relu_mask=P(4096), grad_x=P(), workspace=None, stream=None)
    R("miso_sdf_bwd", bwd + sorted_faults("sorted"), variant="sorted", grid=gg, mlp=m, packed=packed, x=None, sorted=s,
      n=N, grad_sdf=P(), relu_mask=P(4096), grad_x=P(), workspace=P(), stream=None)
    R("miso_sdf_bwd", val("n", ROWS_2GB), variant="tiles_xyz", grid=gg, mlp=m, packed=packed, x=None,
      sorted=binned(TILES_XYZ), n=N, grad_sdf=P(), relu_mask=P(4096), grad_x=P(), workspace=P(), stream=None)
    R("miso_sdf_bwd_rows", bwd + null("x") + off(4, "dfeat_rows") + fld("grid", "flags", 8, 16, 32),
      grid=g, mlp=m, packed=packed, x=P(), n=N, grad_sdf=P(), relu_mask=P(4096), grad_x=P(), dfeat_rows=P(), stream=None)
    R("miso_sdf_bwd_rows", bwd + null("x") + fld("grid", "flags", 16), variant="no_rows", grid=g, mlp=m, packed=packed, x=P(), n=N, grad_sdf=P(),
      relu_mask=P(4096), grad_x=P(), dfeat_rows=None, stream=None)
    loss_in = LOSS_FAULTS + null("loss_slots", "loss_inputs") + off(4, "loss_inputs")
    R("miso_sdf_fwd_loss", fused + loss_in + null("x", "grad_sdf") + val("n_live", P()), variant="x", grid=g, mlp=m,
      packed=packed, x=P(), sorted=None, n=N, **LOSS, loss_inputs=P(), sdf=P(), relu_mask=P(4096), grad_sdf=P(),
      loss_slots=P(4096), n_live=None, stream=None)
    R("miso_sdf_fwd_loss", fused + sorted_faults("sorted") + loss_in + null("grad_sdf"), variant="sorted", grid=g, mlp=m,
      packed=packed, x=None, sorted=s, n=N, **LOSS, loss_inputs=P(), sdf=P(), relu_mask=P(4096), grad_sdf=P(),
      loss_slots=P(4096), n_live=None, stream=None)
    train = fused + loss_in + fld("grid", "ignore_mask", 3)          # no level left whose gradient the step forms
    R("miso_sdf_train", train + null("x") + val("n_live", P()) + val("workspace", P()), variant="x", grid=gg, mlp=m,
      packed=packed, x=P(), sorted=None, n=N, **LOSS, loss_inputs=P(), sdf=P(), loss_slots=P(4096), n_live=None,
      workspace=None, stream=None)
    R("miso_sdf_train", train + sorted_faults("sorted", perm_optional=True) + null("workspace") + off(4, "workspace"),
      variant="sorted", grid=gg, mlp=m, packed=packed, x=None, sorted=s, n=N, **LOSS, loss_inputs=P(), sdf=P(),
      loss_slots=P(4096), n_live=None, workspace=P(), stream=None)
    R("miso_sdf_train", val("n", ROWS_2GB), variant="tiles_xyz", grid=gg, mlp=m, packed=packed, x=None,
      sorted=binned(TILES_XYZ), n=N, **LOSS, loss_inputs=P(), sdf=P(), loss_slots=P(4096), n_live=None, workspace=P(),
      stream=None)
    both = binned()
    both.x_sorted = P()          # with metric points too, the binned step's own "no normalised points" refusal is reached
    R("miso_sdf_train", fld("sorted", "xn_sorted", None), variant="x_sorted", grid=gg, mlp=m, packed=packed, x=None,
      sorted=both, n=N, **LOSS, loss_inputs=P(), sdf=P(), loss_slots=P(4096), n_live=None, workspace=P(), stream=None)
    wg = (null("grid", "mlp", "grads", "grad_sdf", "relu_mask", "workspace") + PK + val("n", -1) + val("flags", 1, 16) +
          grid_faults("grid", True) + fused_faults("grid", "mlp") + fld("grads", "weight[1]", None) + off(4, "workspace") +
          val("workspace_floats", 0))
    R("miso_sdf_wgrad", wg + null("x"), grid=g, mlp=m, packed=packed, x=P(), n=N, grad_sdf=P(), relu_mask=P(4096),
      sorted=None, flags=0, grads=mlp_grad(), workspace=P(), workspace_floats=1 << 24, stream=None)
    R("miso_sdf_wgrad", sorted_faults("sorted")[1:] + val("flags", 1), variant="sorted", grid=g, mlp=m, packed=packed,
      x=None, n=N, grad_sdf=P(), relu_mask=P(4096), sorted=s, flags=16, grads=mlp_grad(), workspace=P(),
      workspace_floats=1 << 24, stream=None)

    # ---- binning and the gradient plan
    R("miso_sort_workspace_bytes", val("n", -1) + val("tiles_per_axis", 0), host=True, n=N, tiles_per_axis=2)
    R("miso_pull_queue_ints", val("n", -1), host=True, n=N)
    sort = (val("n", -1, BIG) + val("tiles_per_axis", 0, 17) + null("workspace", "tile_offsets", "x", "grid") +
            grid_faults("grid", False))
    R("miso_sort_points", sort + null("xn_sorted") + off(4, "xn_sorted"), grid=g, x=P(), n=N, tiles_per_axis=2,
      workspace=P(), x_sorted=None, xn_sorted=P(), perm=P(), tile_offsets=P(), stream=None)
    R("miso_sort_points", null("x_sorted", "perm"), variant="x_sorted", grid=g, x=P(), n=N, tiles_per_axis=2,
      workspace=P(), x_sorted=P(), xn_sorted=None, perm=P(), tile_offsets=P(), stream=None)
    pq = null("grid") + grid_faults("grid", False) + val("tiles_per_axis", 0, 17)
    R("miso_sdf_bwd_scattered_levels", pq, host=True, grid=gg, tiles_per_axis=2, n=20000)
    R("miso_sdf_bwd_push_levels", pq, host=True, grid=gg, tiles_per_axis=2, n=20000)
    R("miso_grad_pull_on_matrix_cores", pq, host=True, grid=gg, tiles_per_axis=2, n=20000, ld_d=F)
    R("miso_grad_pull_levels", pq, host=True, grid=gg, tiles_per_axis=2)
    R("miso_grad_pull_levels", [], variant="tiles_xyz", host=True, grid=gg, tiles_per_axis=TILES_XYZ)
    pull = (sorted_faults("sorted") + null("grid") + val("n", -1) + grid_faults("grid", False) +
            fld("grid", "flags", 1, 2))                          # a level with a buffer that the pull cannot own
    R("miso_grad_pull", pull + null("dfeat") + off(4, "dfeat") + val("ld_d", F + 2, F - 4), grid=gg, sorted=s, n=N,
      dfeat=P(), ld_d=F, rows_in_caller_order=0, stream=None)
    R("miso_grad_pull", val("n", ROWS_2GB), variant="tiles_xyz", grid=gg, sorted=binned(TILES_XYZ), n=N, dfeat=P(), ld_d=F,
      rows_in_caller_order=0, stream=None)
    R("miso_grad_pull_dx", pull + null("grad_feats", "gg_x") + off(4, "grad_feats") + val("ld_g", F + 2, F - 4), grid=gg,
      sorted=s, n=N, grad_feats=P(), ld_g=F, gg_x=P(), stream=None)

    # ---- latent alignment
    R("miso_pair_latent", null("dst_grid", "pose", "out", "coords_src", "feats_src") + off(4, "out") + val("n", -1) +
      LOSS_FAULTS + grid_faults("dst_grid", True) + fld("dst_grid", "flags", 1, 2, 4) + val("ld_feats", F - 1),
      dst_grid=g, pose=P(), coords_src=P(), feats_src=P(), ld_feats=F, n=N, loss_type=2, out=P(), stream=None)
    R("miso_overlap_count", null("pose", "coords_src", "bound_min", "bound_max", "count_out") + val("n", -1, 1 << 24),
      pose=P(), coords_src=P(), n=N, bound_min=LO, bound_max=HI, count_out=P(), stream=None)
    R("miso_align_src_boxes", null("coords", "boxes") + val("n", -1), coords=P(), n=N, boxes=P(), stream=None)
    R("miso_align_plan_bytes", val("n_pairs", -1, 0), host=True, n_pairs=1)
    pair = (fld("pairs", "src", -1, 2) + fld("pairs", "dst", -1, 2, 0) + fld("pairs", "n", -1) + fld("pairs", "gate_n", -1, 1 << 24) +
            fld("pairs", "coords_src", None) + fld("pairs", "feats_src", None) + fld("pairs", "ld_feats", F - 1) +
            grid_faults("pairs", True, pre="dst_grid.") + fld("pairs", "dst_grid.flags", 1, 2, 4))
    cfg = null("cfg") + fld("cfg", "n_pairs", -1) + fld("cfg", "n_submaps", 0, 65)
    R("miso_align_plan_build", cfg + null("pairs", "plan_host") + pair + fld("pairs", "gate_coords", None), host=True,
      pairs=align_pair(), cfg=align_cfg(), plan_host=P(8192))
    R("miso_align_plan_build", fld("pairs", "gate_axis[1]", None) + fld("pairs", "gate_axis[2]", None) +
      fld("pairs", "gate_dims[0]", 0) + fld("pairs", "gate_n", 5), variant="lattice", host=True, pairs=align_pair(True),
      cfg=align_cfg(), plan_host=P(8192))
    R("miso_align_state_layout", val("n_submaps", 0, 65) + val("n_pairs", -1) + val("ring_iters", -1), host=True,
      n_submaps=2, n_pairs=1, ring_iters=4, save_poses=1, offsets=P())
    it = (cfg + fld("cfg", "ring_iters", -1) + fld("cfg", "R0", None) + fld("cfg", "t0", None) + fld("cfg", "state", None) +
          fld("cfg", "plan", None) + fld("cfg", "loss_type", 0, 3) + fld_off(4, "cfg", "state"))
    R("miso_align_iteration_a", it, cfg=align_cfg(True), stream=None)
    R("miso_align_iteration_b", it, cfg=align_cfg(True), stream=None)

    # ---- tracker
    lm = null("R_frame", "out", "coords_frame", "grad_sdf_x", "sdf", "target") + val("n", -1)
    R("miso_lm_normal_eq", lm + val("loss_type", 1, 4), coords_frame=P(), R_frame=P(), grad_sdf_x=P(), sdf=P(), target=P(),
      n=N, loss_type=2, gm_scale=1.0, out=P(), stream=None)
    R("miso_lm_normal_eq", val("gm_scale", 0.0, float("nan")), variant="geman_mcclure", coords_frame=P(), R_frame=P(),
      grad_sdf_x=P(), sdf=P(), target=P(), n=N, loss_type=3, gm_scale=1.0, out=P(), stream=None)

    def track(a, pre, scratch):
        f = fld(a, pre + "n", -1)
        for p in ("R_base", "t_base", "rot_correction", "trans_correction", "pose", "sums", "info", "coords_frame", "target",
                  "coords_world", "sdf", "grad", "relu_mask") + scratch:
            f += fld(a, pre + p, None)
        for p in ("stride_target", "stride_valid", "stride_frame_ids"):
            f += fld(a, pre + p, -1)
        return f + null("grid", a) + fld("grid", "level[0].grad", P()) + fld("grid", "level[1].grad", P())
    # (mlp, packed and the grid's shape are checked by the fused forward, behind the step's first launch: no cases)
    R("miso_lm_track_step", track("args", "", ("ones",)) + fld("args", "loss_type", 1, 4), grid=g, mlp=m, packed=packed,
      args=lm_track(), stream=None)
    a3 = lm_track()
    a3.loss_type = 3
    R("miso_lm_track_step", fld("args", "gm_scale", 0.0), variant="geman_mcclure", grid=g, mlp=m, packed=packed, args=a3,
      stream=None)
    R("miso_track_adam_step", track("args", "s.", ()) + fld("args", "loss_type", 0, 4) + fld("args", "grad_pred", None) +
      fld("args", "adam_table", None) + fld("args", "adam_table_len", 0) + fld("args", "state", None) +
      fld("args", "ring_len", -1) + fld("args", "loss_ring", None), grid=g, mlp=m, packed=packed, args=track_adam(),
      stream=None)
    t3 = track_adam()
    t3.loss_type = 3
    R("miso_track_adam_step", fld("args", "gm_scale", 0.0), variant="geman_mcclure", grid=g, mlp=m, packed=packed, args=t3,
      stream=None)

    # ---- samples, loss, Adam, batch prologue
    R("miso_sample_rays_workspace_bytes", val("n_rays", -1) + val("n_frames", -1), host=True, n_rays=4, n_frames=1)
    rays = null("frames", "sampling", "counts", "pix_h", "pix_w", "u", "g", "workspace", "coords_frame", "sample_frame_ids", "aux")
    rays += val("n_rays", -1, 1 << 29) + off(4, "aux")          # 2^29 rays x 4 rows = 2^31 rows
    rays += fld("sampling", "n_strat", -1, _lib.RAY_MAX_BINS + 1) + fld("sampling", "n_surf", -1) + fld("sampling", "rays_per_frame", 0)
    for p in ("depth", "T_WC", "R_wk", "t_wk"):
        rays += fld("frames", p, None)
    rays += fld("frames", "n_frames", 0) + fld("frames", "H", 0) + fld("frames", "W", 0)
    R("miso_sample_rays", rays, frames=ray_frames(), sampling=ray_sampling(), n_rays=4, pix_b=None, pix_h=P(), pix_w=P(),
      u=P(), g=P(), workspace=P(), coords_frame=P(), sample_frame_ids=P(), aux=P(), pc_world=P(), z_vals=P(), counts=P(),
      stream=None)
    c0 = ray_sampling()
    c0.n_strat = 0
    R("miso_sample_rays", fld("sampling", "n_surf", 0), variant="surface_only", frames=ray_frames(), sampling=c0, n_rays=4,
      pix_b=None, pix_h=P(), pix_w=P(), u=None, g=P(), workspace=P(), coords_frame=P(), sample_frame_ids=P(), aux=P(),
      pc_world=P(), z_vals=P(), counts=P(), stream=None)
    R("miso_mapping_loss", val("n", -1) + LOSS_FAULTS + null("loss_out", "pred", "target", "grad_pred"), **LOSS, pred=P(),
      target=P(), valid=P(), sign=P(), weight=P(), n=N, grad_pred=P(), grad_pred_fs=P(), loss_out=P(), stream=None)
    R("miso_mapping_loss_rows", val("n", -1) + LOSS_FAULTS + null("loss_out", "pred", "loss_rows", "grad_pred") +
      off(4, "loss_rows"), **LOSS, pred=P(), loss_rows=P(), n=N, grad_pred=P(), loss_out=P(), stream=None)
    four, hyper = ("param", "grad", "exp_avg", "exp_avg_sq"), dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
    R("miso_adam_dense", null(*four) + val("numel", -1) + val("step", 0), param=P(), grad=P(), exp_avg=P(), exp_avg_sq=P(),
      numel=8, **hyper, step=1, zero_grad=1, stream=None)
    # miso_adam_step: the per-tensor rules (adam_tensors_ok) on a tensor with `touched`, then the two forms of `when`.
    # One refusal of the entries it replaced has no counterpart by construction: miso_adam_touched(touched = NULL) --
    # here a NULL `touched` means "step by reading the gradient", a valid call.
    tens = null("tensors") + val("n_tensors", 0, _lib.ADAM_MAX_TENSORS + 1) + fld("tensors", "numel", -1)
    for p in four:
        tens += fld("tensors", p, None) + fld_off(4, "tensors", p)
    tens += fld("tensors", "active", None) + fld_off(1, "tensors", "active", "touched")
    R("miso_adam_step", tens + null("when") + fld("when", "step", 0) + fld("when", "table", P()), tensors=adam_tensor(),
      n_tensors=1, when=adam_when(), guard=None, stream=None)      # when.table set, step_dev NULL: neither form
    R("miso_adam_step", tens + null("when") + fld("when", "table", None) + fld("when", "step_dev", None) +
      fld("when", "table_len", 0), variant="device", tensors=adam_tensor(), n_tensors=1, when=adam_when(device=True),
      guard=None, stream=None)                                     # when.table NULL: the host form with step = 0
    no_flags = adam_tensor()
    no_flags.touched = None
    R("miso_adam_step", null("tensors") + fld("tensors", "numel", -1) + fld("tensors", "active", None) +
      [f for p in four for f in fld("tensors", p, None) + fld_off(4, "tensors", p)], variant="by_gradient",
      tensors=no_flags, n_tensors=1, when=adam_when(), guard=None, stream=None)
    R("miso_adam_scalars_table", val("first_step", 0) + val("count", -1) + null("host_out"), host=True, **hyper,
      first_step=1, count=4, host_out=P())
    R("miso_adam_bump", null("step"), step=P(), guard=None, stream=None)
    R("miso_loss_total_bump", null("loss_slots", "total") + val("n_floats", 0), loss_slots=P(4096), n_floats=1024,
      total=P(), step=P(), host_ring=None, ring_len=0, stream=None)
    R("miso_loss_total_bump", null("loss_slots", "total", "step") + val("n_floats", 0) + val("ring_len", 0, 3),
      variant="host_ring", loss_slots=P(4096), n_floats=1024, total=P(), step=P(), host_ring=P(), ring_len=4, stream=None)
    R("miso_mapping_batch", null("R", "t", "table", "frame_ids", "coords_frame", "target", "coords_world", "loss_rows") +
      off(4, "loss_rows") + val("n", -1) + val("n_poses", 0) + val("table_len", 0) +
      [(f"col_strides[{i}]=-1", "col_strides", int64s(*[-1 if j == i else 1 for j in range(4)])) for i in range(4)],
      R=P(), t=P(), n_poses=1, table=P(), table_len=1, frame_ids=P(), coords_frame=P(), target=P(), valid=P(), sign=P(),
      weight=P(), col_strides=int64s(1, 1, 1, 1), valid_is_bool=0, n=N, coords_world=P(), loss_rows=P(), sanitize=0,
      stream=None)
    R("miso_rigid_by_index", null("R", "idx", "x", "y") + val("n", -1) + val("n_poses", 0), R=P(), t=P(), idx=P(), x=P(), n=N,
      n_poses=1, transpose=0, y=P(), stream=None)
    R("miso_grid_pool_avg", null("coords", "features", "bound_min", "pooled", "counts") + val("n", -1) + val("d", 0) +
      val("nx", 0, 1 << 23) + val("ny", 0) + val("nz", 0) + val("cell_size", 0.0, float("nan")) + val("ld_features", 3),
      coords=P(), features=P(), n=N, d=4, ld_features=4, bound_min=LO, cell_size=0.5, nx=8, ny=8, nz=8, pooled=P(),
      counts=P(), stream=None)

    # ---- voxel down-sampling
    R("miso_voxel_down_workspace_bytes", val("capacity", -1, 1 << 22), host=True, capacity=64)
    R("miso_voxel_down_sample", val("capacity", -1, 1 << 22) + val("ld", 2) + val("voxel_size", 0.0, INF, float("nan")) +
      null("out_count", "points", "workspace", "out_idx") + off(4, "workspace"), points=P(1024), ld=3, capacity=64,
      n_live=None, voxel_size=0.1, workspace=P(8192), out_idx=P(1024), out_count=P(), stream=None)
    sel = dict(src_coords=P(1024), src_ids=P(1024), src_aux=P(1024), out_idx=P(1024), out_count=P(), capacity=64,
               dst_coords=P(1024), dst_ids=P(1024), dst_aux=P(1024), live_rows=P(), stream=None)
    R("miso_voxel_select_rows", val("capacity", -1, 1 << 22) + null("src_coords", "src_ids", "src_aux", "out_idx",
      "out_count", "dst_coords", "dst_ids", "dst_aux", "live_rows") + off(4, "src_aux", "dst_aux") +
      [(f"{d} is {s_}", d, sel[s_]) for d, s_ in (("dst_coords", "src_coords"), ("dst_ids", "src_ids"), ("dst_aux", "src_aux"))],
      **sel)

    # ---- nearest neighbours, ICP
    np_, ws = nn_plan(), P(8192)
    IDX = null("workspace") + off(4, "workspace")
    R("miso_nn_plan", null("plan", "bound_min", "bound_max") + val("n_tgt", -1, BIG) + val("max_rings", -1, 65) +
      val("cell", 0.0, INF, float("nan")) + [("bound_max[1]=inf", "bound_max", floats(1, INF, 1)),
      ("bound_max[1]<bound_min[1]", "bound_max", floats(1, -1, 1)), ("bound_max[2]=nan", "bound_max", floats(1, 1, float("nan"))),
      ("bound_min[1]=-inf", "bound_min", floats(0, -INF, 0)), ("extent[0]=inf", "bound_min", floats(-3e38, 0, 0)),
      ("n_tgt=0", "n_tgt", 0), ("cell doubled", "cell", 1e30)],
      host=True, bound_min=LO, bound_max=floats(3e38, 1, 1), cell=1e36, n_tgt=10, max_rings=8, plan=_lib.NnPlan())
    R("miso_nn_workspace_bytes", plan_faults("plan", "nn"), host=True, plan=np_)
    R("miso_nn_build", plan_faults("plan", "nn") + val("ld", 2) + null("tgt") + IDX, plan=np_, tgt=P(), ld=3, workspace=ws,
      stream=None)
    q = plan_faults("plan", "nn") + val("ld", 2) + val("n", -1, BIG) + IDX
    R("miso_nn_query", q + null("stats", "src", "out_d2", "out_idx"), plan=np_, workspace=ws, src=P(), ld=3, n=N, out_d2=P(),
      out_idx=P(), stats=P(), stream=None)
    ap = (val("m", -1, BIG) + val("n", -1, BIG) + val("ld_t", 2) + val("ld_s", 2) + null("tgt", "src", "out_d2", "out_idx"))
    R("miso_nn_all_pairs", ap, tgt=P(), ld_t=3, m=4, src=P(), ld_s=3, n=N, out_d2=P(), out_idx=P(), stream=None)
    K = val("k", 0, _lib.NN_KNN_MAX + 1)
    R("miso_nn_knn", q + K + null("stats", "src", "out_d2", "out_idx"), plan=np_, workspace=ws, src=P(), ld=3, n=N, k=3,
      out_d2=P(), out_idx=P(), stats=P(), stream=None)
    R("miso_nn_knn_all_pairs", ap + K, tgt=P(), ld_t=3, m=4, src=P(), ld_s=3, n=N, k=3, out_d2=P(), out_idx=P(), stream=None)
    R("miso_nn_knn_normals", q + K + null("pts", "normals", "counts"), plan=np_, workspace=ws, pts=P(), ld=3, n=N, k=3,
      normals=P(), counts=P(), stream=None)
    R("miso_nn_normals", q + null("pts", "normals", "counts") + val("radius", 0.0, 1e30, float("nan")), plan=np_,
      workspace=ws, pts=P(), ld=3, n=N, radius=0.5, normals=P(), counts=P(), stream=None)
    R("miso_icp_transform", val("n", -1, BIG) + val("ld", 2) + null("pose", "src", "out"), src=P(), ld=3, n=N, pose=P(),
      out=P(), stream=None)
    R("miso_icp_workspace_bytes", val("n", -1), host=True, n=N)
    R("miso_icp_sums", val("n", -1, BIG) + val("m", -1, BIG) + val("ld_t", 2) + null("workspace", "out", "moved", "d2", "idx",
      "tgt", "normals") + off(4, "workspace", "out") + val("kind", -1, 2) + val("loss", -1, 2) +
      val("max_dist", -1.0, float("nan")) + val("tukey_k", 0.0) + val("ld_n", 2), moved=P(), d2=P(), idx=P(), n=N, tgt=P(),
      ld_t=3, m=4, normals=P(), ld_n=3, max_dist=1.0, kind=1, loss=1, tukey_k=1.0, origin=None, workspace=P(8192), out=P(),
      stream=None)

    # ---- triangle meshes
    mp, mws, lists = mesh_plan(), P(8192), P()
    cap = val("capacity", -1, _lib.MESH_MAX_ENTRIES + 1)
    index = plan_faults("plan", "mesh") + IDX + null("lists") + cap
    rays = val("ld_o", 2) + val("ld_d", 2) + val("n", -1, BIG) + null("origins", "dirs")
    arrays = val("n_vert", -1) + val("n_tri", -1, BIG) + val("ld_v", 2) + val("ld_t", 2) + null("verts", "tris")
    R("miso_mesh_plan", null("plan", "bound_min", "bound_max") + val("n_tri", -1, BIG, 0) + val("cell", 0.0, INF) +
      [("bound_max[1]<bound_min[1]", "bound_max", floats(1, -1, 1))], host=True, bound_min=LO, bound_max=HI, cell=0.25, n_tri=4,
      plan=_lib.MeshPlan())
    R("miso_mesh_workspace_bytes", plan_faults("plan", "mesh"), host=True, plan=mp)
    R("miso_mesh_count", plan_faults("plan", "mesh") + val("ld_v", 2) + val("ld_t", 2) + val("n_vert", -1) +
      null("entries", "tris", "verts") + off(4, "entries") + IDX, plan=mp, verts=P(), ld_v=3, n_vert=4, tris=P(), ld_t=3,
      workspace=mws, entries=P(), stream=None)
    R("miso_mesh_build", index, plan=mp, workspace=mws, lists=lists, capacity=16, stream=None)
    R("miso_mesh_cast_rays", index + rays + null("out_t", "out_tri") + off(4, "stats"), plan=mp, workspace=mws, lists=lists,
      capacity=16, origins=P(), ld_o=3, dirs=P(), ld_d=3, n=N, t_min=0.0, t_max=INF, out_t=P(), out_tri=P(), stats=P(),
      stream=None)
    R("miso_mesh_cast_rays_all", arrays + rays + null("out_t", "out_tri"), verts=P(), ld_v=3, n_vert=4, tris=P(), ld_t=3,
      n_tri=4, origins=P(), ld_o=3, dirs=P(), ld_d=3, n=N, t_min=0.0, t_max=INF, out_t=P(), out_tri=P(), stream=None)
    far = [(lab.replace("plan", "plan_far").replace("workspace", "workspace_far").replace("lists", "lists_far")
            .replace("capacity", "capacity_far"), a + "_far", v) for lab, a, v in index if lab != "plan=NULL"]
    pts = val("ld_p", 2) + val("n", -1, BIG) + null("pts", "out_d2", "out_tri") + off(4, "out_vw")
    R("miso_mesh_closest", index + far + fld("plan_far", "n_tri", 5) + fld("plan_far", "reserved", -1) + pts + off(4, "stats"),
      plan=mp, workspace=mws, lists=lists, capacity=16, plan_far=mesh_plan(2.0), workspace_far=P(8192), lists_far=P(),
      capacity_far=16, pts=P(), ld_p=3, n=N, out_d2=P(), out_tri=P(), out_vw=P(), stats=P(), stream=None)
    R("miso_mesh_closest", val("workspace_far", P()) + val("lists_far", P()) + val("capacity_far", 1), variant="no_far",
      plan=mp, workspace=mws, lists=lists, capacity=16, plan_far=None, workspace_far=None, lists_far=None, capacity_far=0,
      pts=P(), ld_p=3, n=N, out_d2=P(), out_tri=P(), out_vw=P(), stats=P(), stream=None)
    R("miso_mesh_closest_all", arrays + pts, verts=P(), ld_v=3, n_vert=4, tris=P(), ld_t=3, n_tri=4, pts=P(), ld_p=3, n=N,
      out_d2=P(), out_tri=P(), out_vw=P(), stream=None)
    R("miso_mesh_count_hits", index + rays + null("out_count"), plan=mp, workspace=mws, lists=lists, capacity=16, origins=P(),
      ld_o=3, dirs=P(), ld_d=3, n=N, t_min=0.0, t_max=INF, out_count=P(), stream=None)
    R("miso_mesh_count_hits_all", arrays + rays + null("out_count"), verts=P(), ld_v=3, n_vert=4, tris=P(), ld_t=3, n_tri=4,
      origins=P(), ld_o=3, dirs=P(), ld_d=3, n=N, t_min=0.0, t_max=INF, out_count=P(), stream=None)

    # ---- atlas
    R("miso_atlas_plan_bytes", val("n_submaps", 0), host=True, n_submaps=2)
    two = (_lib.Grid * 2)(grid(), grid())
    R("miso_atlas_plan_build", null("grids", "plan_host") + val("n_submaps", 0, 4097) +
      [(lab.replace("grids.", "grids[1]."), a, v) for lab, a, v in grid_faults("grids", True, pre="[1].")] +
      fld("grids", "[1].flags", 4) + fld("grids", "[0].level[0].sX", 5) + fld("grids", "[1].n_levels", 1) +
      fld("grids", "[1].level[1].C", 8), host=True, grids=two, n_submaps=2, plan_host=P(16384))
    atlas = null("plan", "poses", "shape", "mlp") + val("n_submaps", 0) + val("flags", 1, 1 << 20) + PK
    atlas += grid_faults("shape", False) + fused_faults("shape", "mlp", vec4=False)[1:]
    base = dict(plan=P(16384), n_submaps=2, shape=g, poses=P(), mlp=m, packed=packed)
    lattice = dict(axis_x=None, axis_y=None, axis_z=None, nx=0, ny=0, nz=0)
    R("miso_atlas_sdf_fwd", atlas + val("n", -1) + val("ld_feats", F - 1), **base, x=P(), n=N, **lattice, sdf=P(), feats=P(),
      ld_feats=F, flags=0, stream=None)
    R("miso_atlas_sdf_fwd", null("feats") + fld("shape", "level[1].C", 8) + fld("shape", "n_levels", 5),
      variant="feats_only", plan=P(16384), n_submaps=2, shape=g, poses=P(), mlp=None, packed=None, x=P(), n=N, **lattice,
      sdf=None, feats=P(), ld_feats=F, flags=0, stream=None)
    R("miso_atlas_sdf_fwd", null("axis_x", "axis_y", "axis_z") + val("nx", 0, 2) + val("ny", 0) + val("nz", 0),
      variant="lattice", **base, x=None, n=N, axis_x=P(), axis_y=P(), axis_z=P(), nx=1, ny=1, nz=N, sdf=P(), feats=None,
      ld_feats=0, flags=0, stream=None)
    R("miso_atlas_bwd_supported", null("shape", "mlp") + grid_faults("shape", False) + fld("shape", "flags", 4) +
      fused_faults("shape", "mlp", vec4=False)[1:] + val("n_submaps", 0, _lib.ATLAS_BWD_MAX_SUBMAPS + 1), host=True,
      shape=g, mlp=m, n_submaps=2, want_poses=1)
    R("miso_atlas_bwd_workspace_bytes", val("n", 0), host=True, n=N, n_submaps=2)
    R("miso_atlas_sdf_bwd", atlas + val("n", -1) + val("n_submaps", _lib.ATLAS_BWD_MAX_SUBMAPS + 1) +
      null("x", "gsdf", "workspace") + off(1, "workspace"), **base, x=P(), n=N, gsdf=P(), gx=P(), gposes=P(), workspace=P(),
      flags=0, stream=None)
    R("miso_atlas_sphere_trace", atlas + null("origins", "dirs", "points", "hit") + val("n_rays", -1) + val("max_iters", 0) +
      val("fd_step", 0.0, float("nan")), **base, origins=P(), dirs=P(), n_rays=N, min_dist=0.0, max_dist=4.0, max_iters=8,
      epsilon=1e-3, fd_step=1e-3, points=P(), hit=P(), sdf=P(), steps=P(), grad=P(), flags=0, stream=None)

    # ---- marching cubes
    dims = val("nx", 0, 1 << 25) + val("ny", 0) + val("nz", 0)          # 2^25 x 8 x 8 = 2^31 samples
    R("miso_mc_words", dims, host=True, nx=8, ny=8, nz=8)
    R("miso_mc_workspace_bytes", dims, host=True, nx=8, ny=8, nz=8)
    R("miso_mc_classify", dims + null("vol", "workspace", "counts") + off(4, "workspace"), vol=P(2048), nx=8, ny=8, nz=8,
      iso=0.0, workspace=P(), counts=P(2048), stream=None)
    R("miso_mc_emit", dims + null("workspace", "offsets", "faces") + val("n_tri_chunks", -1, 65) + val("capacity_tris", -1),
      nx=8, ny=8, nz=8, workspace=P(), offsets=P(2048), n_tri_chunks=4, capacity_tris=4, faces=P(), stream=None)
    R("miso_mc_vertices", dims + null("vol", "workspace", "offsets", "verts") + val("n_vert_chunks", -1, 65) +
      val("capacity_verts", -1), vol=P(2048), nx=8, ny=8, nz=8, iso=0.0, workspace=P(), offsets=P(2048), n_vert_chunks=4,
      capacity_verts=4, verts=P(), stream=None)
    R("miso_mc_case_table", null("table_host"), host=True, table_host=P(4096))


build_recipes()
VALUE_ONLY = ("miso_version", "miso_error_string")      # no refusals: counted through their values


# ---- calling ---------------------------------------------------------------------------------------------------------------
def _pass(argtype, v, keep):
    if isinstance(v, (C.Structure, C.Array)):
        v = _clone(v)                                  # a call may write its struct (cfg, plan): never the recipe's
        keep.append(v)
        return C.cast(C.pointer(v), argtype) if isinstance(v, C.Array) else C.byref(v)
    if isinstance(v, int) and not isinstance(v, bool) and hasattr(argtype, "contents"):
        return C.cast(C.c_void_p(v), argtype)          # an address where the ABI names a struct pointer
    return v


def _call(lib, name, args):
    res, argtypes = _lib.SIGNATURES[name]
    assert len(argtypes) == len(args), f"{name}: {len(args)} arguments for {len(argtypes)}"
    keep = []
    rc = getattr(lib, name)(*[_pass(t, v, keep) for t, v in zip(argtypes, args.values())])
    return rc, keep


def _hex(obj):
    return bytes(obj).hex()


def _valid_result(lib, name, args):
    """the valid call of a host query: its value, with what it wrote where that is the answer"""
    rc, keep = _call(lib, name, args)
    if name in ("miso_nn_plan", "miso_mesh_plan"):
        return [rc, _hex(keep[-1])]
    if name == "miso_align_plan_build":
        cfg = keep[1]
        return [rc, cfg.vec4, cfg.max_n, cfg.max_gate_n, cfg.max_gate_rows]
    if name == "miso_align_state_layout":
        return [rc, list((C.c_int64 * 12).from_address(args["offsets"]))]
    return rc


def cases():
    """name -> thunk(lib) giving the code or value of the case; in a fixed order"""
    out = {}

    def add(key, fn):
        assert key not in out, f"duplicate case {key}"
        out[key] = fn

    add("miso_version:prefix", lambda lib: lib.miso_version().decode().split("src=")[0])
    for code in (0, 2001, 2002, 2003):
        add(f"miso_error_string:{code}", lambda lib, code=code: lib.miso_error_string(code).decode())
    for name, variant, args, faults in RECIPES:
        head = name + ("/" + variant if variant else "")
        if name in HOST:
            add(head + ":valid", lambda lib, name=name, args=args: _valid_result(lib, name, args))
        for label, arg, new in faults:
            assert arg in args, f"{head}: no argument {arg}"
            changed = dict(args)
            changed[arg] = new(args[arg]) if callable(new) else new
            if name in ("miso_nn_plan", "miso_mesh_plan") and arg != "plan":      # a second valid plan, or a refusal
                add(f"{head}:{label}", lambda lib, name=name, a=changed: _valid_result(lib, name, a))
            else:
                add(f"{head}:{label}", lambda lib, name=name, a=changed: _call(lib, name, a)[0])
    return out


def launching(key):
    return key.split(":")[0].split("/")[0] not in HOST.union(VALUE_ONLY)


def run(lib, only_refusals_may_launch=True):
    got = {}
    for key, thunk in cases().items():
        got[key] = thunk(lib)
        if only_refusals_may_launch and launching(key) and got[key] not in REFUSALS:
            raise SystemExit(f"{key} returned {got[key]}: not a refusal -- the case reached (or would reach) a launcher; "
                             "take it out of the cases")
    return got


def coverage_gaps():
    covered = {n for n, *_ in RECIPES}.union(VALUE_ONLY)
    return sorted(set(_lib.SIGNATURES) - covered), sorted(covered - set(_lib.SIGNATURES))


def record():
    """Run every case against the library MISO_HIP_LIB names (default: the tree's) and write the golden file.  Meant for
    a build of the commit whose behaviour is kept; never for a machine with a GPU (a case that is no refusal launches)."""
    import torch
    assert not torch.cuda.is_available(), "record on a machine without a GPU: a case that is no refusal would launch"
    missing, unknown = coverage_gaps()
    assert not missing and not unknown, (missing, unknown)
    got = run(_lib.load())
    with open(GOLDEN, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(got)} cases of {len(set(_lib.SIGNATURES))} entry points -> {GOLDEN} ({_lib.LIB_PATH})")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        raise SystemExit(__doc__)
    record()
