"""MIPS-Fusion's alignment baseline, fused loop against op-by-op loop, on 8 ScanNet-shaped submaps and 28 pairs
(tools/bench_extras.scannet_atlas: the cfg-4 alignment case).  Both routes are align_multiple_submaps_mips of the same
commit on the same one-batch dataset -- every row a surface row -- in alternating repeats from the same perturbed poses;
per constraint and per iteration the median and the range over the repeats are printed as one JSON line and written to
profiles/align_mips.json.  The op-by-op loop is the reference's own op sequence (grid_opt/align/mips.py) and is the
baseline: there is no target ratio.

    python tools/bench_align_mips.py [--rows 20000] [--repeats 3] [--fused-iters 24] [--loop-iters 3] [--out FILE]

The fused figure is given twice: the iterations proper (what base.fused_alignment_loop times: staging, warm-up and graph
capture excluded) and the whole call divided by its iterations (everything included).  The op-by-op figure is the
whole call divided by its iterations; it has no set-up to speak of."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class SurfaceBatch(torch.utils.data.Dataset):
    """One batch in keyframe frames: ``rows`` samples per submap inside its bound (every submap has one keyframe, at
    identity), all of them on the measured surface (sdf 0: the reference's |gt| < 1e-3 keeps every row)."""

    def __init__(self, n_submaps, rows, bound):
        g = torch.Generator().manual_seed(77)
        n = n_submaps * rows
        lo, hi = bound[:, 0], bound[:, 1]
        self.mi = {"coords_frame": torch.rand(n, 3, generator=g) * (hi - lo) + lo,
                   "sample_frame_ids": torch.arange(n_submaps).repeat_interleave(rows).view(n, 1),
                   "weights": torch.ones(n, 1)}
        self.gt = {"sdf": torch.zeros(n, 1), "sdf_valid": torch.ones(n, 1), "sdf_signs": torch.zeros(n, 1)}

    def __len__(self):
        return 1

    def __getitem__(self, i):
        return self.mi, self.gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20000, help="surface samples per submap in the batch")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--fused-iters", type=int, default=24)
    ap.add_argument("--loop-iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_mips.json"))
    args = ap.parse_args()
    from bench import SCANNET_CFG, scannet_atlas      # (tools/bench_extras.py, reached through bench as tools do)
    import miso_amd.grid_opt.align.miso as AM
    import miso_amd.grid_opt.align.mips as MP
    dev = "cuda:0"
    S = 8
    atlas = scannet_atlas(dev, S)
    for s in range(1, S):      # one pretrained decoder for all submaps, as the demos load it
        atlas.get_submap(s).decoder.load_state_dict(atlas.get_submap(0).decoder.state_dict())
    why = AM.fused_sdf_refusal(atlas, dev)
    if why is not None:
        raise SystemExit(f"the fused route does not cover this case: {why}")
    ds = SurfaceBatch(S, args.rows, torch.tensor(SCANNET_CFG["grid"]["bound"]))
    start = [(atlas.rotation_corrections[s].detach().clone(), atlas.translation_corrections[s].detach().clone())
             for s in range(S)]

    def run(fused, iters, constraint):
        with torch.no_grad():
            for s in range(S):
                atlas.rotation_corrections[s].copy_(start[s][0])
                atlas.translation_corrections[s].copy_(start[s][1])
        atlas.no_fused_alignment = not fused
        atlas.__dict__.pop("_last_align_loop", None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        MP.align_multiple_submaps_mips(atlas, ds, num_iters=iters - 1, lr=1e-3, constraint_type=constraint, device=dev,
                                       verbose=False)
        torch.cuda.synchronize()
        whole = (time.perf_counter() - t0) / iters
        if not fused:
            return whole, whole
        lp = atlas.__dict__["_last_align_loop"]      # (KeyError: the fused route did not run)
        return lp["seconds"] / max(lp["iterations"], 1), whole

    def stat(v):
        return {"median_ms": statistics.median(v) * 1e3, "min_ms": min(v) * 1e3, "max_ms": max(v) * 1e3}

    out = {"case": f"{S} ScanNet-shaped submaps, {S * (S - 1) // 2} pairs, {args.rows} surface rows per submap, "
                   "overlap gate on",
           "repeats": args.repeats, "fused_iterations": args.fused_iters, "op_by_op_iterations": args.loop_iters,
           "device": torch.cuda.get_device_name(0)}
    for constraint in ("point_to_plane", "point_to_point"):
        run(True, 8, constraint), run(False, 1, constraint)       # warm-up: code objects, allocator, caches
        fused, fused_whole, loop = [], [], []
        for _ in range(args.repeats):                             # alternating
            a, b = run(True, args.fused_iters, constraint)
            fused.append(a), fused_whole.append(b)
            loop.append(run(False, args.loop_iters, constraint)[0])
        out[constraint] = {"fused_per_iteration": stat(fused), "fused_per_iteration_with_setup": stat(fused_whole),
                           "op_by_op_per_iteration": stat(loop),
                           "fused_slowest_ahead_of_op_by_op_fastest": max(fused_whole) < min(loop)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
