"""The k nearest neighbours of a sampled surface among itself, and normals from them, at the shape of
utils_scannet.align_mesh_to_ref: --samples (10^6) surface samples of the 8 x 6 x 3 m room, k = 30 (Open3D's
estimate_normals default).  Routes on identical seeded clouds, alternating:

 neighbour lists
  a  the cell list: ops.NearestIndex.knn on an index built once (the build is timed on its own: align_mesh_to_ref builds
     it anyway), default cell and rings
  b  ops.knn_all_pairs, the first --reduced queries only (every block scans every target: the full cloud would take
     samples / reduced times as long); a == b bit for bit is recorded for those queries
  c  torch on the device: chunked torch.cdist + topk on the same --reduced queries, chunks held under 2 GB
  d  scipy.spatial.cKDTree.query(k=30, workers=16) on all queries where scipy is importable (null otherwise), clouds
     and results on the host
 normals
  e  NearestIndex.normals(knn=30)
  f  NearestIndex.normals(), today's default radius of NN_NORMAL_SPACINGS point spacings
 and the share of queries that the rings leave to the all-pairs kernel (the counters of a).

Times are host wall clock between two device synchronisations, median (min .. max) over --repeats alternating repeats
after a warm-up; a route whose run takes more than a second is repeated --slow_repeats times.

    python tools/bench_knn.py [--out profiles/knn.json]"""
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


def cloud(samples, dev, seed):
    from miso_amd.grid_opt.utils import utils_eval, utils_sdf
    room = utils_sdf.box_mesh(ROOM)
    g = torch.Generator(device=dev).manual_seed(seed)
    pts, _, _ = utils_eval.sample_surface(torch.from_numpy(room.vertices).to(dev), torch.from_numpy(room.triangles).to(dev), samples, g)
    return pts.to(torch.float32).contiguous()


def cdist_topk(src, tgt, k):
    rows = max(1, min(src.shape[0], int(2e9 // (4 * max(tgt.shape[0], 1)))))
    d2 = torch.empty((src.shape[0], k), device=src.device)
    idx = torch.empty((src.shape[0], k), device=src.device, dtype=torch.int64)
    for a in range(0, src.shape[0], rows):
        d, j = torch.cdist(src[a:a + rows], tgt).topk(k, dim=1, largest=False)
        d2[a:a + rows], idx[a:a + rows] = d * d, j
    return d2, idx


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
    ap.add_argument("--samples", type=int, default=1000000)
    ap.add_argument("--reduced", type=int, default=16384, help="queries of the all-pairs and the torch route")
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--slow_repeats", type=int, default=2)
    ap.add_argument("--routes", nargs="*", default=["build", "a", "b", "c", "d", "e", "f"])
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from miso_amd import _lib, ops
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    dev = "cuda:0"
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    pts = cloud(args.samples, dev, seed=args.samples)
    few = pts[:args.reduced].contiguous()
    index = ops.NearestIndex(pts)
    k = args.k
    routes = {"build": lambda: ops.NearestIndex(pts), "a": lambda: index.knn(pts, k), "b": lambda: ops.knn_all_pairs(few, pts, k),
              "c": lambda: cdist_topk(few, pts, k), "e": lambda: index.normals(knn=k), "f": lambda: index.normals()}
    if cKDTree is not None:
        def d():
            p = pts.cpu().numpy()
            return cKDTree(p).query(p, k=k, workers=16)
        routes["d"] = d
    routes = {r: fn for r, fn in routes.items() if r in args.routes}
    first = {r: timed(fn) for r, fn in routes.items()}                          # also the warm-up
    entry = {"samples": int(pts.shape[0]), "k": k, "reduced_queries": int(few.shape[0]), "cell": index.cell, "dims": list(index.dims),
             "max_rings": ops.NN_MAX_RINGS}
    if "a" in first:
        ad2, aidx, stats = first["a"][1]
        stats = stats.tolist()
        entry["stats"] = stats
        entry["share_to_all_pairs"] = stats[1] / max(sum(stats), 1)
        if "b" in first:
            bd2, bidx = first["b"][1]
            entry["a_equals_b_bit_for_bit_on_reduced"] = bool(torch.equal(ad2[:few.shape[0]].view(torch.int32), bd2.view(torch.int32))
                                                              and torch.equal(aidx[:few.shape[0]], bidx))
        if "c" in first:
            entry["c_indices_differing_from_a"] = int((first["c"][1][1] != aidx[:few.shape[0]]).sum())
    if "e" in first and "f" in first:
        (ne, ce), (nf, cf) = first["e"][1], first["f"][1]
        cos = (ne * nf).sum(dim=1).abs().clamp(max=1.0)
        entry["radius_neighbours_mean"] = float(cf.float().mean())
        entry["angle_knn_to_radius_normals_median_rad"] = float(torch.acos(cos).median())
    slow = {r: first[r][0] > 1000.0 for r in routes}
    times = {r: [] for r in routes}
    for i in range(args.repeats):                           # alternate: every route sees the same state of the machine
        for r, fn in routes.items():
            if not slow[r] or i < args.slow_repeats:
                times[r].append(timed(fn)[0])
    for r in ("build", "a", "b", "c", "d", "e", "f"):
        entry[r] = spread(times[r]) if r in times else None
    scale = pts.shape[0] / max(few.shape[0], 1)
    for r in ("b", "c"):
        if entry[r]:
            entry[r]["median_ms_scaled_to_all_queries"] = entry[r]["median_ms"] * scale
    print(json.dumps(entry), file=sys.stderr)
    out = {"workload": "surface samples of the 8 x 6 x 3 m room among themselves; wall clock between device synchronisations; "
                       "routes alternate; b and c on the first `reduced_queries` queries only",
           "library": _lib.load().miso_version().decode(), "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
           "slow_repeats": args.slow_repeats, "result": entry,
           "defaults": {"NN_CELL_SPACINGS": ops.NN_CELL_SPACINGS, "NN_MAX_RINGS": ops.NN_MAX_RINGS,
                        "NN_NORMAL_SPACINGS": ops.NN_NORMAL_SPACINGS, "NN_KNN_MAX": ops.NN_KNN_MAX}}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
