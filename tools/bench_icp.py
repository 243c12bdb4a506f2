"""One iteration of utils_scannet.align_mesh_to_ref's point-to-plane ICP on the evaluation room shape, three routes on
identical seeded clouds, alternating:

  a  the kernels: ops.IcpWorkspace.step (miso_icp_transform, miso_nn_query on one ops.NearestIndex, miso_icp_sums, one read
     of 32 doubles) + the float64 solve on the host
  b  the same loop with the same index search, the transform and the sums done by torch ops on the device: (N, 6) float64
     Jacobian rows, J^T W J and J^T W r by matrix products, one read of the 6 x 7 system
  c  scipy.spatial.cKDTree on 16 workers + numpy float64 where scipy is importable (null otherwise), clouds on the host

Workload: the demo's 8 x 6 x 3 m room, its six rectangles sampled twice with --points samples (utils_eval.sample_surface),
the source moved by 2 degrees / 4 cm, the target with its face normals; the coarse pass (L2, max_dist 0.3) and the fine
pass (Tukey k = 0.01, max_dist 0.03), --iters iterations each from the same start, time per iteration.  The index is
built once outside the timed region for a and b, the k-d tree once for c, as a registration call does.

Times are host wall clock between two device synchronisations, median (min .. max) over --repeats alternating repeats after
a warm-up; a route whose run takes more than a second is repeated --slow_repeats times.  Also recorded: the poses the
three routes end at agree.

    python tools/bench_icp.py [--out profiles/icp.json]"""
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


def small_pose(deg=2.0, metres=0.04):
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(deg)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = np.array([2.0, -1.0, 1.0]) / np.sqrt(6.0) * metres
    return T


def clouds(points, dev):
    """(source, target, target face normals) on the device, fp32; the source is the room moved by the inverse of small_pose()"""
    from miso_amd.grid_opt.utils import utils_scannet, utils_sdf
    room = utils_sdf.box_mesh(ROOM)
    moved = utils_sdf.TriangleMesh(room.vertices.copy(), room.triangles).apply_transform(np.linalg.inv(small_pose()))
    src, _ = utils_scannet._sampled(moved, points, 0, dev, False)
    tgt, normals = utils_scannet._sampled(room, points, 1, dev, True)
    return src, tgt, normals


def torch_sums(moved, d2, idx, tgt, normals, max_dist, k):
    ok = (idx >= 0) & (d2.to(torch.float64) <= max_dist * max_dist)
    p, j = moved[ok].to(torch.float64), idx[ok]
    q, n = tgt[j].to(torch.float64), normals[j].to(torch.float64)
    r = ((p - q) * n).sum(dim=1)
    J = torch.cat([torch.cross(p, n, dim=1), n], dim=1)
    w = torch.ones_like(r) if k is None else torch.where(r.abs() <= k, (1.0 - (r / k) ** 2) ** 2, torch.zeros_like(r))
    Jw = J * w[:, None]
    return torch.cat([Jw.T @ J, (Jw.T @ r)[:, None]], dim=1).cpu().numpy()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def spread(t, iters):
    t = np.asarray(t) / iters
    return {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()), "repeats": int(len(t))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--slow_repeats", type=int, default=3)
    ap.add_argument("--routes", nargs="*", default=["a", "b", "c"])
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from miso_amd import _lib, ops
    from miso_amd.grid_opt.utils import utils_registration as reg
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    dev = torch.device("cuda:0")
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    src, tgt, normals = clouds(args.points, dev)
    index = ops.NearestIndex(tgt)
    work = ops.IcpWorkspace(src, index, normals)
    d2b, idxb = torch.empty_like(work.search[0]), torch.empty_like(work.search[1])
    search_b = (d2b, idxb, torch.empty(2, device=dev, dtype=torch.int32))
    host = None
    if cKDTree is not None and "c" in args.routes:
        host = dict(src=src.cpu().numpy().astype(np.float64), tgt=tgt.cpu().numpy().astype(np.float64),
                    normals=normals.cpu().numpy().astype(np.float64))
        host["tree"] = cKDTree(host["tgt"])
    results = []
    for name, max_dist, k, init in (("coarse", 0.3, None, np.eye(4)), ("fine", 0.03, 1e-2, None)):
        if init is None:
            init = reg.registration_icp(src, index, tgt, normals, 0.3, np.eye(4), max_iteration=30).transformation

        def a():
            T = init.copy()
            for _ in range(args.iters):
                T = reg.solve_point_to_plane(work.step(T, max_dist, "point_to_plane", k)) @ T
            return T

        def b():
            T = init.copy()
            for _ in range(args.iters):
                T32 = torch.from_numpy(T).to(device=dev, dtype=torch.float32)
                moved = src @ T32[:3, :3].T + T32[:3, 3]
                d2, idx, _ = index.query(moved, out=search_b)
                s = torch_sums(moved, d2, idx, tgt, normals, max_dist, k)
                T = reg.transform_vector6d_to_matrix4d(np.linalg.solve(s[:, :6], -s[:, 6])) @ T
            return T

        def c():
            T = init.copy()
            for _ in range(args.iters):
                p = host["src"] @ T[:3, :3].T + T[:3, 3]
                d, j = host["tree"].query(p, workers=16)
                ok = d <= max_dist
                p, q, n = p[ok], host["tgt"][j[ok]], host["normals"][j[ok]]
                r = ((p - q) * n).sum(axis=1)
                J = np.concatenate([np.cross(p, n), n], axis=1)
                w = np.ones(len(r)) if k is None else np.where(np.abs(r) <= k, (1.0 - (r / k) ** 2) ** 2, 0.0)
                T = reg.transform_vector6d_to_matrix4d(np.linalg.solve(J.T @ (J * w[:, None]), -(J.T @ (w * r)))) @ T
            return T

        routes = {r: fn for r, fn in (("a", a), ("b", b), ("c", c)) if r in args.routes and (r != "c" or host is not None)}
        first = {r: timed(fn) for r, fn in routes.items()}                      # also the warm-up
        slow = {r: first[r][0] > 1000.0 for r in routes}
        times = {r: [] for r in routes}
        for rep in range(args.repeats):                     # alternate: every route sees the same state of the machine
            for r, fn in routes.items():
                if not slow[r] or rep < args.slow_repeats:
                    times[r].append(timed(fn)[0])
        entry = {"pass": name, "max_dist": max_dist, "tukey_k": k, "iterations_timed": args.iters,
                 "source_points": int(src.shape[0]), "target_points": int(tgt.shape[0]),
                 "pose_error_to_truth_m": {r: float(np.linalg.norm(first[r][1][:3, 3] - small_pose()[:3, 3])) for r in routes},
                 "largest_pose_entry_difference_to_a": {r: float(np.abs(first[r][1] - first["a"][1]).max())
                                                        for r in routes if "a" in routes}}
        for r in ("a", "b", "c"):
            entry[r + "_per_iteration"] = spread(times[r], args.iters) if r in times else None
        results.append(entry)
        print(json.dumps(entry), file=sys.stderr)
    out = {"workload": "8 x 6 x 3 m room surfaces sampled twice, source moved by 2 deg / 4 cm, point-to-plane with face normals; "
                       "wall clock between device synchronisations per iteration; routes alternate",
           "library": _lib.load().miso_version().decode(), "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "slow_repeats": args.slow_repeats, "results": results}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
