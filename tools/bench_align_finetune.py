"""The SDF fine-tune stage of alignment, fused loop against op-by-op loop, on 8 ScanNet-shaped submaps and 28 pairs
(tools/bench_extras.scannet_atlas: the cfg-4 alignment case).  Both routes run generic_align_multiple_submaps with the
same pair loss on the same one-batch dataset, in alternating repeats from the same perturbed poses; per iteration the
median and the range over the repeats are printed as one JSON line and written to profiles/align_finetune.json.

    python tools/bench_align_finetune.py [--rows 20000] [--repeats 3] [--fused-iters 24] [--loop-iters 3]

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


class OneBatch(torch.utils.data.Dataset):
    """One batch in keyframe frames: ``rows`` samples per submap inside its bound (every submap has one keyframe, at
    identity), 15 % of them invalid, measured SDF ~ N(0, 0.1)."""

    def __init__(self, n_submaps, rows, bound):
        g = torch.Generator().manual_seed(77)
        n = n_submaps * rows
        lo, hi = bound[:, 0], bound[:, 1]
        self.mi = {"coords_frame": torch.rand(n, 3, generator=g) * (hi - lo) + lo,
                   "sample_frame_ids": torch.arange(n_submaps).repeat_interleave(rows).view(n, 1),
                   "weights": torch.ones(n, 1)}
        self.gt = {"sdf": 0.1 * torch.randn(n, 1, generator=g),
                   "sdf_valid": (torch.rand(n, 1, generator=g) > 0.15).float(),
                   "sdf_signs": torch.zeros(n, 1)}

    def __len__(self):
        return 1

    def __getitem__(self, i):
        return self.mi, self.gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20000, help="samples per submap in the batch")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--fused-iters", type=int, default=24)
    ap.add_argument("--loop-iters", type=int, default=3)
    ap.add_argument("--loss", default="L2", choices=["L2", "L1", "GM"])
    args = ap.parse_args()
    from bench import SCANNET_CFG, scannet_atlas      # (tools/bench_extras.py, reached through bench as tools do)
    import miso_amd.grid_opt.align.base as AB
    import miso_amd.grid_opt.align.miso as AM
    dev = "cuda:0"
    S = 8
    atlas = scannet_atlas(dev, S)
    for s in range(1, S):      # one pretrained decoder for all submaps, as the demos load it
        atlas.get_submap(s).decoder.load_state_dict(atlas.get_submap(0).decoder.state_dict())
    why = AM.fused_sdf_refusal(atlas, dev)
    if why is not None:
        raise SystemExit(f"the fused route does not cover this case: {why}")
    ds = OneBatch(S, args.rows, torch.tensor(SCANNET_CFG["grid"]["bound"]))
    start = [(atlas.rotation_corrections[s].detach().clone(), atlas.translation_corrections[s].detach().clone())
             for s in range(S)]

    def run(fused, iters):
        with torch.no_grad():
            for s in range(S):
                atlas.rotation_corrections[s].copy_(start[s][0])
                atlas.translation_corrections[s].copy_(start[s][1])
        atlas.no_fused_alignment = not fused
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn = AM.sdf_finetune_loss(atlas, AM.draw_batches(ds, 1, dev), align_loss=args.loss, device=dev)
        AB.generic_align_multiple_submaps(atlas, ds, ("sdf", fn), num_iters=iters - 1, lr=1e-3, verbose=False)
        torch.cuda.synchronize()
        whole = (time.perf_counter() - t0) / iters
        if not fused:
            return whole, whole
        lp = atlas.__dict__["_last_align_loop"]
        return lp["seconds"] / max(lp["iterations"], 1), whole

    run(True, 8), run(False, 1)                                   # warm-up: code objects, allocator, caches
    fused, fused_whole, loop = [], [], []
    for _ in range(args.repeats):                                 # alternating
        a, b = run(True, args.fused_iters)
        fused.append(a), fused_whole.append(b)
        loop.append(run(False, args.loop_iters)[0])

    def stat(v):
        return {"median_ms": statistics.median(v) * 1e3, "min_ms": min(v) * 1e3, "max_ms": max(v) * 1e3}
    out = {"case": f"{S} ScanNet-shaped submaps, {S * (S - 1) // 2} pairs, {args.rows} rows per submap, loss {args.loss}, "
                   "overlap gate on",
           "repeats": args.repeats, "fused_iterations": args.fused_iters, "op_by_op_iterations": args.loop_iters,
           "fused_per_iteration": stat(fused), "fused_per_iteration_with_setup": stat(fused_whole),
           "op_by_op_per_iteration": stat(loop),
           "fused_slowest_ahead_of_op_by_op_fastest": max(fused_whole) < min(loop),
           "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "align_finetune.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
