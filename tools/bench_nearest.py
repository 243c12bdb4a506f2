"""Both directions of a Chamfer evaluation's nearest-neighbour search, four routes on identical seeded clouds, alternating:

  a  the cell list: ops.NearestIndex (build, one read of the bounds) + query, once per direction, default cell and rings
  b  ops.nearest_all_pairs, both directions
  c  torch on the device: chunked torch.cdist + min, chunks held under 2 GB (what a user could write without the kernels)
  d  scipy.spatial.cKDTree on 16 workers where scipy is importable (null otherwise), clouds and results on the host

Workloads: the demo's 8 x 6 x 3 m room, its six rectangles sampled (utils_eval.sample_surface) and centroid-down-sampled
(utils_geometry.voxel_centroid_down_sample) -- `eval`: 1 000 000 samples at 0.02 m, the evaluation shape; `fine`: --fine_samples
at 0.005 m; `small`: 30 000 points; and three tiny pairs around the size where ops.nearest changes route.  The prediction
is the ground truth displaced by 1 cm noise, 2 % of it moved up to 1 m away.

Times are host wall clock between two device synchronisations, median (min .. max) over --repeats alternating repeats after
--warmup; a route whose run takes more than a second is repeated --slow_repeats times.  Also recorded: a == b bit for bit,
the counters of a, and on `eval` the sweep of cell in {1, 2, 4} x voxel and max_rings in {2, 4, 8, 16} behind the defaults,
and the mean number of targets in a query's cell and in its 27 cells of rings 0 and 1.

    python tools/bench_nearest.py [--out profiles/nearest.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOM = np.array([[0.0, 8.0], [0.0, 6.0], [0.0, 3.0]])


def clouds(samples, voxel, dev, seed, keep=None):
    """(prediction, ground truth) on the device, fp32"""
    from miso_amd.grid_opt.utils import utils_eval, utils_geometry, utils_sdf
    room = utils_sdf.box_mesh(ROOM)
    v, f = room.vertices, room.triangles
    g = torch.Generator(device=dev).manual_seed(seed)
    pts, _, _ = utils_eval.sample_surface(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), samples, g)
    gt = utils_geometry.voxel_centroid_down_sample(pts, voxel).to(torch.float32) if voxel > 0 else pts.to(torch.float32)
    if keep is not None and gt.shape[0] > keep:
        gt = gt[torch.randperm(gt.shape[0], device=dev, generator=g)[:keep]]
    pred = gt + 0.01 * torch.randn(gt.shape, device=dev, generator=g)
    out = torch.rand(gt.shape[0], device=dev, generator=g) < 0.02
    shift = torch.randn(gt.shape, device=dev, generator=g)
    shift = shift / shift.norm(dim=1, keepdim=True) * torch.rand((gt.shape[0], 1), device=dev, generator=g)
    pred = torch.where(out[:, None], pred + shift, pred)
    return pred.contiguous(), gt.contiguous()


def cdist_route(src, tgt):
    rows = max(1, min(src.shape[0], int(2e9 // (4 * max(tgt.shape[0], 1)))))
    d2 = torch.empty(src.shape[0], device=src.device)
    idx = torch.empty(src.shape[0], device=src.device, dtype=torch.int64)
    for a in range(0, src.shape[0], rows):
        d, j = torch.cdist(src[a:a + rows], tgt).min(dim=1)
        d2[a:a + rows], idx[a:a + rows] = d * d, j
    return d2, idx


def candidates(index, src):
    """Mean number of targets in a query's own cell, and in the 27 cells of rings 0 and 1 (where most queries finish)"""
    lo = torch.tensor(list(index.plan.bound_min), device=src.device)
    dx, dy, dz = index.dims
    hi = torch.tensor([dx - 1, dy - 1, dz - 1], device=src.device, dtype=torch.float32)
    cell = torch.tensor(index.cell, device=src.device)

    def cells(p):
        c = torch.minimum(torch.clamp(torch.floor(torch.div(p - lo, cell)), min=0.0), hi).long()
        return (c[:, 2] * dy + c[:, 1]) * dx + c[:, 0]

    pop = torch.bincount(cells(index.tgt), minlength=dx * dy * dz).reshape(1, 1, dz, dy, dx).float()
    box = torch.nn.functional.avg_pool3d(pop, 3, stride=1, padding=1, count_include_pad=True) * 27.0
    q = cells(src)
    return float(pop.reshape(-1)[q].mean()), float(box.reshape(-1)[q].mean())


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def spread(t):
    t = np.asarray(t)
    return {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()), "repeats": int(len(t))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--slow_repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fine_samples", type=int, default=2000000)
    ap.add_argument("--workloads", nargs="*", default=["tiny1k", "tiny3k", "tiny10k", "small", "eval", "fine"])
    ap.add_argument("--no_sweep", action="store_true")
    ap.add_argument("--routes", nargs="*", default=["a", "b", "c", "d"], help="a alone: what a kernel trace is taken of")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from miso_amd import _lib, ops
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    dev = "cuda:0"
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    shapes = {"tiny1k": (20000, 0.0, 1000), "tiny3k": (20000, 0.0, 3000), "tiny10k": (40000, 0.0, 10000),
              "small": (100000, 0.0, 30000), "eval": (1000000, 0.02, None), "fine": (args.fine_samples, 0.005, None)}
    results, sweep = [], []
    for name in args.workloads:
        samples, voxel, keep = shapes[name]
        pred, gt = clouds(samples, voxel, dev, seed=len(name) + samples, keep=keep)

        def a():
            return ops.NearestIndex(gt).query(pred), ops.NearestIndex(pred).query(gt)

        def b():
            return ops.nearest_all_pairs(pred, gt), ops.nearest_all_pairs(gt, pred)

        def c():
            return cdist_route(pred, gt), cdist_route(gt, pred)

        def d():
            p, g = pred.cpu().numpy(), gt.cpu().numpy()
            return cKDTree(g).query(p, workers=16), cKDTree(p).query(g, workers=16)

        routes = {"a": a, "b": b, "c": c}
        if cKDTree is not None:
            routes["d"] = d
        routes = {r: fn for r, fn in routes.items() if r in args.routes}
        if list(routes) == ["a"]:
            for _ in range(args.repeats):
                timed(a)
            continue
        first = {r: timed(fn) for r, fn in routes.items()}                      # also the warm-up
        (ad2p, aip, stp), (ad2g, aig, stg) = first["a"][1]
        (bd2p, bip), (bd2g, big) = first["b"][1]
        same = bool(torch.equal(ad2p.view(torch.int32), bd2p.view(torch.int32)) and torch.equal(aip, bip) and
                    torch.equal(ad2g.view(torch.int32), bd2g.view(torch.int32)) and torch.equal(aig, big))
        entry = {"workload": name, "pred_points": int(pred.shape[0]), "gt_points": int(gt.shape[0]),
                 "a_equals_b_bit_for_bit": same,
                 "c_indices_differing_from_a": int((first["c"][1][0][1] != aip).sum()) if "c" in first else None,
                 "stats_pred_to_gt": stp.tolist(), "stats_gt_to_pred": stg.tolist(),
                 "cell_gt_index": ops.NearestIndex(gt).cell, "max_rings": ops.NN_MAX_RINGS}
        if int(np.prod(ops.NearestIndex(gt).dims)) <= 1 << 24:
            entry["candidates_own_cell_and_rings_0_1"] = candidates(ops.NearestIndex(gt), pred)
        slow = {r: first[r][0] > 1000.0 for r in routes}
        for _ in range(max(args.warmup - 1, 0)):
            for r, fn in routes.items():
                if not slow[r]:
                    timed(fn)
        times = {r: [] for r in routes}
        for k in range(args.repeats):                       # alternate: every route sees the same state of the machine
            for r, fn in routes.items():
                if not slow[r] or k < args.slow_repeats:
                    times[r].append(timed(fn)[0])
        for r in ("a", "b", "c", "d"):
            entry[r] = spread(times[r]) if r in times else None
        entry["a_ahead_of_b_and_c_beyond_spread"] = (bool(entry["a"]["max_ms"] < min(entry["b"]["min_ms"], entry["c"]["min_ms"]))
                                                     if entry["c"] else None)
        results.append(entry)
        print(json.dumps(entry), file=sys.stderr)
        if name == "eval" and not args.no_sweep:
            for mult in (1, 2, 4):
                for rings in (2, 4, 8, 16):
                    def run():
                        return (ops.NearestIndex(gt, cell=mult * voxel, max_rings=rings).query(pred),
                                ops.NearestIndex(pred, cell=mult * voxel, max_rings=rings).query(gt))
                    timed(run)
                    t = [timed(run)[0] for _ in range(5)]
                    (_, _, s1), (_, _, s2) = run()
                    sweep.append({"cell": mult * voxel, "max_rings": rings, **spread(t), "to_all_pairs": int(s1[1]) + int(s2[1]),
                                  "candidates_own_cell_and_rings_0_1": candidates(ops.NearestIndex(gt, cell=mult * voxel), pred)})
                    print(json.dumps(sweep[-1]), file=sys.stderr)
    out = {"workload": "8 x 6 x 3 m room surfaces, prediction = ground truth + 1 cm noise, 2 % moved up to 1 m; both directions; "
                       "wall clock between device synchronisations; routes alternate",
           "library": _lib.load().miso_version().decode(), "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "slow_repeats": args.slow_repeats, "results": results, "sweep_eval": sweep,
           "defaults": {"NN_CELL_SPACINGS": ops.NN_CELL_SPACINGS, "NN_MAX_RINGS": ops.NN_MAX_RINGS,
                        "NN_ALL_PAIRS_BELOW": ops.NN_ALL_PAIRS_BELOW}}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
