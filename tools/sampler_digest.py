"""dev: one SHA-256 per output tensor of every entry point whose kernel samples a feature grid (csrc/trilinear.hpp) --
run it at two commits on one card and compare the lists: a change of the sampler's text must not change a bit.

Inputs, all seeded: two levels (5x4x3 and 9x7x6 vertices), C = 4 and 8, channels-last (and NCDHW for the generic encode
kernels), the four flag sets, 193 points (three wavefronts and a partial one) with points outside the bound, on both
faces and one NaN row.  Whatever is summed with float atomics (grid gradients, the atlas pose gradient) is taken on a
second set: one point per every second cell of the coarse level, so that no vertex receives two contributions and no sum
depends on the order of the atomics (and a single wavefront, so the pose sums of the atlas backward have one order).
pair_latent: 193 vertices are one workgroup (launch_pair_latent: 2048 per workgroup), one fp64 atomic per sum.

The binned calls (the sort, the binned forward / backward / training step, the pull in each of its forms, the push, the
batched pair stage) run three times on the same inputs: an output whose three runs agree bit for bit is recorded by its
digest, one whose runs differ -- sums ordered by LDS or float atomics -- as "not reproducible run to run", which is then
what both commits must say.  The sort leaves the order inside a tile to its atomics, so the binned batch is put into a
canonical order first (every tile's points by their original index) and is in the list itself: equal lists mean that
both commits worked on the same binned batch.

    python tools/sampler_digest.py [--out digests.json]"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from miso_amd import _lib, ops  # noqa: E402

DEV = torch.device("cuda:0")
SIZES = ((3, 4, 5), (6, 7, 9))      # (Z, Y, X) per level
BOUND = ((-1.0, 1.5), (0.0, 2.0), (-0.5, 0.7))
FLAGS = {"default": 0, "align_corners": _lib.F_ALIGN_CORNERS, "pad_border": _lib.F_PAD_BORDER,
         "normalized": _lib.F_COORDS_NORMALIZED}
OUT = {}


def put(name, t):
    if t is None:
        return
    torch.cuda.synchronize()
    OUT[name] = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def features(C, channels_last, seed=1):
    fs = [rnd(seed + l, 1, C, *s).to(DEV) for l, s in enumerate(SIZES)]
    return [f.contiguous(memory_format=torch.channels_last_3d) if channels_last else f for f in fs]


def points(flags, scatter):
    """(n,3) points for a flag set; normalised coordinates under COORDS_NORMALIZED, else inside BOUND."""
    lo, hi = torch.tensor([b[0] for b in BOUND]), torch.tensor([b[1] for b in BOUND])
    if scatter:      # continuous index i + 0.3 in cells i = 0, 2 (x, y), 0 (z) of the coarse level, + outside + NaN
        Z, Y, X = SIZES[0]
        def xn(i, size):
            ix = i + 0.3
            return 2 * ix / (size - 1) - 1 if flags & _lib.F_ALIGN_CORNERS else (2 * ix + 1) / size - 1
        p = torch.tensor([[xn(i, X), xn(j, Y), xn(0, Z)] for i in (0, 2) for j in (0, 2)] + [[1.5, 0.0, 0.0]] +
                         [[float("nan")] * 3], dtype=torch.float32)
    else:
        p = torch.rand(193, 3, generator=torch.Generator().manual_seed(7)) * 2.4 - 1.2      # some outside
        p[0], p[1], p[2] = -1.0, 1.0, torch.tensor([-1.0, 1.0, 0.25])                       # on the faces
        p[100] = float("nan")
    return (p if flags & _lib.F_COORDS_NORMALIZED else lo + (p + 1) * 0.5 * (hi - lo)).to(DEV)


def encode(tag, feats, meta, x, xs):
    F = sum(f.shape[1] for f in feats)
    gout, ggx, gouts, ggxs = (rnd(11, 193, F).to(DEV), rnd(12, 193, 3).to(DEV), rnd(13, len(xs), F).to(DEV),
                              rnd(14, len(xs), 3).to(DEV))
    ggf = [rnd(20 + l, *f.shape).to(DEV).contiguous(memory_format=torch.channels_last_3d if f.stride(1) == 1 else
                                                    torch.contiguous_format) for l, f in enumerate(feats)]
    none, both = [False] * len(feats), [True] * len(feats)
    put(tag + "/fwd", ops.encode_fwd_raw(x, feats, meta))
    for form in ("lean", "weights"):
        os.environ.pop("MISO_ENCODE_NO_LEAN", None)
        if form == "weights":
            os.environ["MISO_ENCODE_NO_LEAN"] = "1"
        put(f"{tag}/bwd.gx/{form}", ops.encode_bwd_raw(x, feats, meta, gout, True, none)[0])
        for gg in (None, ggf):
            o, gx, _ = ops.encode_bwd2_raw(x, feats, meta, gout, ggx, gg, True, none)
            put(f"{tag}/bwd2.ggF/{form}/gg={gg is not None}", o)
            put(f"{tag}/bwd2.gx/{form}/gg={gg is not None}", gx)
    os.environ.pop("MISO_ENCODE_NO_LEAN", None)
    gx, grads = ops.encode_bwd_raw(xs, feats, meta, gouts, True, both)
    o, gx2, grads2 = ops.encode_bwd2_raw(xs, feats, meta, gouts, ggxs, ggf, True, both)
    for n, t in [("bwd.gx", gx), ("bwd2.ggF", o), ("bwd2.gx", gx2)] + [(f"bwd.grad{l}", g) for l, g in enumerate(grads)] + \
            [(f"bwd2.grad{l}", g) for l, g in enumerate(grads2)]:
        put(f"{tag}/scatter/{n}", t)


def decoder(F, H):
    ws = [rnd(31, H, F) * 0.5, rnd(32, H, H) * 0.2, rnd(33, 1, H) * 0.3]
    return ops.DecoderPack([w.to(DEV) for w in ws], [rnd(34 + i, w.shape[0]).to(DEV) * 0.1 for i, w in enumerate(ws)])


def fused(tag, feats, meta, pack, x, xs):
    none, both = [False] * len(feats), [True] * len(feats)
    sdf, mask = ops.sdf_fwd_raw(x, feats, meta, pack, True)
    gsdf = rnd(41, 193, 1).to(DEV)
    put(tag + "/sdf_fwd.sdf", sdf), put(tag + "/sdf_fwd.mask", mask)
    put(tag + "/sdf_bwd.gx", ops.sdf_bwd_raw(x, feats, meta, pack, gsdf, mask, True, none)[0])
    gx, _, rows = ops.sdf_bwd_rows_raw(x, feats, meta, pack, gsdf, mask, True, none)
    put(tag + "/sdf_bwd_rows.gx", gx), put(tag + "/sdf_bwd_rows.rows", rows)
    gw, gb = ops.sdf_wgrad_raw(x, feats, meta, pack, gsdf, mask)
    for i, t in enumerate(gw + gb):
        put(f"{tag}/sdf_wgrad.{i}", t)
    # the scattering calls, on the collision-free set
    n = len(xs)
    _, masks = ops.sdf_fwd_raw(xs, feats, meta, pack, True)
    gs = rnd(42, n, 1).to(DEV)
    gx, grads = ops.sdf_bwd_raw(xs, feats, meta, pack, gs, masks, True, both)
    gxr, gradsr, rows = ops.sdf_bwd_rows_raw(xs, feats, meta, pack, gs, masks, True, both)
    lin = torch.cat((rnd(43, n, 1) * 0.1, torch.ones(n, 3)), 1).to(DEV).contiguous()
    slots = torch.zeros(_lib.LOSS_SLOTS, 2, device=DEV)
    gradt, sdft = [torch.zeros_like(f) for f in feats], torch.empty(n, 1, device=DEV)
    ops.sdf_train_unsorted_raw(xs, feats, meta, pack, lin, slots, gradt, sdf_out=sdft)
    for nme, t in [("sdf_bwd.gx", gx), ("sdf_bwd_rows.gx", gxr), ("sdf_bwd_rows.rows", rows), ("sdf_train.sdf", sdft),
                   ("sdf_train.loss", slots)] + [(f"sdf_bwd.grad{l}", g) for l, g in enumerate(grads)] + \
            [(f"sdf_bwd_rows.grad{l}", g) for l, g in enumerate(gradsr)] + [(f"sdf_train.grad{l}", g) for l, g in enumerate(gradt)]:
        put(f"{tag}/scatter/{nme}", t)


def atlas(tag, C, meta, pack, x, xs):
    fs = [features(C, True, seed=1), features(C, True, seed=5)]
    metas, q = [meta, meta], ops.AtlasQuery()
    c, s = 0.9553365, 0.2955202      # a rotation about z and a shift; the scatter set: both submaps in the world frame
    poses = torch.tensor([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], [c, -s, 0, s, c, 0, 0, 0, 1, 0.1, -0.2, 0.05]],
                         dtype=torch.float32, device=DEV)
    eye = poses[:1].repeat(2, 1).contiguous()
    sdf, feats = q(fs, metas, poses, pack, x=x, want_feats=True)
    put(tag + "/atlas.sdf", sdf), put(tag + "/atlas.feats", feats)
    exact, no = ops._EXACT_F32, [[False] * 2] * 2
    put(tag + "/atlas_bwd.gx", q._backward(fs, metas, poses, pack, x, rnd(51, 193, 1).to(DEV), True, False, no, exact)[0])
    gx, gp, grads = q._backward(fs, metas, eye, pack, xs, rnd(52, len(xs), 1).to(DEV), True, True, [[True] * 2] * 2, exact)
    for nme, t in [("gx", gx), ("gposes", gp)] + [(f"grad{i}.{l}", g) for i, gs in enumerate(grads) for l, g in enumerate(gs)]:
        put(f"{tag}/scatter/atlas_bwd.{nme}", t)
    d = torch.nn.functional.normalize(rnd(53, 193, 3), dim=1).to(DEV)
    pts, hit, ex = q.trace(fs, metas, poses, pack, x, d, min_dist=0.0, max_dist=3.0, max_iters=12, epsilon=1e-3,
                           want_sdf=True, want_steps=True, grad_step=1e-2)
    for nme, t in [("points", pts), ("hit", hit)] + sorted(ex.items()):
        put(f"{tag}/trace.{nme}", t)


def pair(tag, feats, meta, x):
    F = sum(f.shape[1] for f in feats)
    c, s = 0.9800666, 0.1986693
    Rs = torch.tensor([[c, -s, 0], [s, c, 0], [0, 0, 1.0]], device=DEV)
    for loss in ("L1", "L2"):
        P = [Rs.clone(), torch.tensor([[0.05], [-0.1], [0.02]], device=DEV), torch.eye(3, device=DEV),
             torch.tensor([[-0.03], [0.04], [0.0]], device=DEV)]
        for t in P:
            t.requires_grad_(True)
        val = ops.pair_latent(*P, x, rnd(61, 193, F).to(DEV), feats, meta, loss)
        val.backward()
        put(f"{tag}/pair_latent.{loss}", val)
        for i, t in enumerate(P):
            put(f"{tag}/pair_latent.{loss}.g{i}", t.grad)


def repeatable(name, fn, runs=3):
    """fn() -> [(label, tensor)]: the digest of every tensor whose `runs` runs agree, else that they do not"""
    seen = {}
    for _ in range(runs):
        for label, t in fn():
            torch.cuda.synchronize()
            seen.setdefault(label, set()).add(hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest())
    for label, digests in seen.items():
        OUT[f"{name}/{label}"] = digests.pop() if len(digests) == 1 else "not reproducible run to run"


def binned(tag, C, pack, tiles):
    """8192 points (a uniform cloud and a clump: the push's crowd of >= 100 per tile at 4 tiles per axis) on 8^3, 16^3
    and 32^3 vertices, binned at `tiles` per axis: 4 -- even bricks, the block kernel -- or 5 -- the wavefront kernel."""
    n, sizes = 8192, (8, 16, 32)
    feats = [rnd(70 + l, 1, C, s, s, s).mul_(0.1).to(DEV).contiguous(memory_format=torch.channels_last_3d)
             for l, s in enumerate(sizes)]
    meta = ops.GridMeta.from_bound(BOUND)
    lo, hi = torch.tensor([b[0] for b in BOUND]), torch.tensor([b[1] for b in BOUND])
    u = torch.rand(n, 3, generator=torch.Generator().manual_seed(71))
    u[n // 2:] = 0.4 + 0.1 * u[n // 2:]
    x = (lo + u * (hi - lo)).to(DEV)
    sb = ops.SortedBatch(n, DEV, tiles=tiles)

    def sort_canonical():
        sb.sort(x, meta)
        ends = sb.tile_offsets.long()[1:].contiguous()
        tile = torch.searchsorted(ends, torch.arange(n, device=DEV), right=True)
        order = torch.argsort(tile * n + sb.perm.long())
        sb.xn_sorted.copy_(sb.xn_sorted[order])
        sb.perm.copy_(sb.perm[order])
        return [(k, getattr(sb, k)) for k in ("xn_sorted", "perm", "tile_offsets")]

    repeatable(tag + "/sort", sort_canonical)
    rows = rnd(72, n, 3 * C).to(DEV)
    every = [True] * 3
    for form, env in (("mc", {}), ("vector", {"MISO_PULL_MC": "0"}),
                      ("vector_no_split", {"MISO_PULL_MC": "0", "MISO_PULL_NO_SPLIT": "1"})):
        os.environ.update(env)
        try:
            repeatable(f"{tag}/pull/{form}", lambda: [(f"grad{l}", g) for l, g in enumerate(
                ops.grad_pull_raw(feats, meta, sb, rows, [torch.empty_like(f) for f in feats]))])
        finally:
            for k in env:
                os.environ.pop(k)
    lin = torch.cat((rnd(73, n, 1) * 0.1, torch.ones(n, 3)), 1).to(DEV).contiguous()

    def two_launches():
        slots, mask = torch.zeros(_lib.LOSS_SLOTS, 2, device=DEV), ops.sdf_mask_buffer(pack, n, DEV)
        gpred, sdf = torch.empty(n, device=DEV), torch.empty(n, 1, device=DEV)
        ops.sdf_fwd_loss_raw(feats, meta, pack, sb, lin, mask, gpred, slots, sdf_out=sdf)
        _, grads = ops.sdf_bwd_raw(x, feats, meta, pack, gpred, mask, False, every, sorted_batch=sb, overwrite=True,
                                   gsdf_sorted=True)
        return [("loss", slots), ("sdf", sdf), ("gsdf", gpred), ("mask", mask), ("rows", sb._ws[:n * 3 * C].clone())] + \
               [(f"grad{l}", g) for l, g in enumerate(grads)]

    def one_launch():
        slots, sdf = torch.zeros(_lib.LOSS_SLOTS, 2, device=DEV), torch.empty(n, 1, device=DEV)
        grads = [torch.empty_like(f) for f in feats]
        ops.sdf_train_raw(feats, meta, pack, sb, lin, slots, grads, sdf_out=sdf)
        return [("loss", slots), ("sdf", sdf), ("rows", sb._ws[:n * 3 * C].clone())] + [(f"grad{l}", g) for l, g in enumerate(grads)]

    for exact in (False, True):
        with ops.exact_fp32(exact):
            form = "exact" if exact else "split"
            repeatable(f"{tag}/fwd_loss+bwd/{form}", two_launches)
            repeatable(f"{tag}/train/{form}", one_launch)


def pair_stage(tag, C, gate):
    """The batched pair stage (AlignPlan.iteration_a) of three submaps and their six pairs: 1500 source vertices per pair
    are one workgroup; with gate points the launch is pair_stage_kernel, without them pair_latent_batch_kernel."""
    feats, meta = features(C, True), ops.GridMeta.from_bound(BOUND)
    lo, hi = torch.tensor([b[0] for b in BOUND]), torch.tensor([b[1] for b in BOUND])
    coords = (lo + torch.rand(1500, 3, generator=torch.Generator().manual_seed(81)) * (hi - lo)).to(DEV)
    fsrc = rnd(82, 1500, 2 * C).to(DEV)
    R0 = torch.eye(3).repeat(3, 1, 1).to(DEV)
    t0 = torch.tensor([[0.0, 0.0, 0.0], [0.3, -0.2, 0.1], [-0.4, 0.5, 0.2]]).reshape(3, 3, 1).to(DEV)
    descr = [dict(src=a, dst=b, coords=coords, feats_src=fsrc, feats_dst=feats, meta_dst=meta,
                  gate_pts=coords[:700].contiguous() if gate else None) for a in range(3) for b in range(3) if a != b]

    def stage():
        plan = ops.AlignPlan(R0, t0, descr, loss_type="L2")
        plan.params[1, :3] = torch.tensor([0.02, -0.01, 0.03], device=DEV)
        plan.iteration_a()
        return [("pair_out", plan.pair_out.clone()), ("overlap_counts", plan.overlap_counts.clone())]

    repeatable(f"{tag}/gate={gate}", stage)


def run(tag, fn, *args):
    """a flag set or layout that an entry point refuses is recorded as such (the refusal has to stay the same too)"""
    try:
        fn(tag, *args)
    except _lib.MisoError as e:
        OUT[f"{tag}/{fn.__name__}"] = f"refused: {e.what} code {e.code}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    for fname, flags in FLAGS.items():
        meta = ops.GridMeta.from_bound(BOUND, flags=flags)
        x, xs = points(flags, False), points(flags, True)
        for C in (4, 8):
            for cl in (True, False):
                tag = f"{fname}/C{C}/{'cl' if cl else 'ncdhw'}"
                run(tag, encode, features(C, cl), meta, x, xs)
                run(tag, pair, features(C, cl), meta, x)
            feats, pack = features(C, True), decoder(2 * C, 32 if C == 4 else 64)
            for exact in (False, True):
                with ops.exact_fp32(exact):
                    tag = f"{fname}/C{C}/{'exact' if exact else 'split'}"
                    run(tag, fused, feats, meta, pack, x, xs)
                    run(tag, atlas, C, meta, pack, x, xs)
    for C in (4, 8):
        pack = decoder(3 * C, 64)
        for tiles in (4, 5):
            run(f"binned/C{C}/tiles{tiles}", binned, C, pack, tiles)
        for gate in (False, True):
            run(f"pair_stage/C{C}", pair_stage, C, gate)
    for k in sorted(OUT):
        print(OUT[k], k)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(OUT, open(a.out, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
