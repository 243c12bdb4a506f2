"""Forward + backward of atlas(x).sum() under autograd: the one-launch route (GridAtlas.fused_backward ->
ops.AtlasQuery.differentiable: miso_atlas_sdf_fwd + miso_atlas_sdf_bwd) against the per-submap loop of this same commit
(fused_backward off), gradients to the points, the submap pose corrections and every submap's features.

Workloads: the 8 ScanNet-shaped submaps of bench.py at 540 000 world points drawn over the atlas's bound with a margin
(points inside several, one and no submap), and the 3-submap ATLAS golden case at its 1024 points.

    python tools/bench_atlas_grad.py [--repeats 20] [--out profiles/atlas_grad_bench.json]

Prints one JSON line: per workload the median and spread (min .. max) of both routes in ms (HIP events around
zero_grad + forward + backward), their ratio, and the largest difference of the two routes' gradients."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def unlock_all(atlas):
    for s in range(atlas.num_submaps):
        atlas.unlock_submap(s)
    atlas.unlock_submap_pose()
    return atlas


def step(atlas, x, fused):
    atlas.fused_backward = fused
    atlas.zero_grad(set_to_none=True)
    x.grad = None
    atlas(x).sum().backward()


def timed(atlas, x, fused):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    step(atlas, x, fused)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def gradients(atlas, x):
    return [x.grad.clone()] + [p.grad.clone() for p in atlas.params_for_all_submap_poses()] + \
        [p.grad.clone() for p in atlas.params_for_all_features()]


def measure(name, atlas, x, repeats, warmup):
    x = x.clone().requires_grad_(True)
    for _ in range(warmup):
        step(atlas, x, True)
    got = gradients(atlas, x)
    for _ in range(warmup):
        step(atlas, x, False)
    want = gradients(atlas, x)
    worst = max((a - b).abs().max().item() / max(b.abs().max().item(), 1e-30) for a, b in zip(got, want))
    times = {"fused": [], "loop": []}
    for _ in range(repeats):                          # alternate, so that both see the same state of the machine
        for k in times:
            times[k].append(timed(atlas, x, k == "fused"))
    atlas.fused_backward = False
    out = {"workload": name, "points": int(x.shape[0]), "submaps": atlas.num_submaps,
           "max_gradient_difference_rel": worst}
    for k, t in times.items():
        t = np.asarray(t)
        out[k] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max())}
    out["speedup_median"] = out["loop"]["median_ms"] / out["fused"]["median_ms"]
    # faster by more than the run-to-run spread of this run: the slowest fused repeat against the fastest loop repeat
    out["fused_faster_beyond_spread"] = bool(out["fused"]["max_ms"] < out["loop"]["min_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=540000)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import bench
    import golden_cases as gc
    from test_grid_opt_mirror import make_atlas_two_kf
    from miso_amd import _lib
    dev = "cuda:0"
    results = []
    atlas = unlock_all(bench.scannet_atlas(dev, 8))
    gb = atlas.global_bound(device="cpu").detach()
    gen = torch.Generator().manual_seed(11)
    x = ((gb[:, 0] - 1.0) + (gb[:, 1] - gb[:, 0] + 2.0) * torch.rand(args.points, 3, generator=gen)).to(dev)
    results.append(measure("8 ScanNet-shaped submaps (bench.scannet_atlas)", atlas, x, args.repeats, args.warmup))
    del atlas
    small = unlock_all(make_atlas_two_kf(dev))
    xs = torch.from_numpy(gc.atlas_world_points()).to(dev)
    results.append(measure("ATLAS golden case (3 submaps, C=4, L=2, H=64)", small, xs, args.repeats, args.warmup))
    out = {"library": _lib.load().miso_version().decode(), "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "timed": "zero_grad + forward + backward of atlas(x).sum(), HIP events",
           "results": results}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
