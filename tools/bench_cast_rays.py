"""First-hit ray casting against a mesh, three routes on the same rays, alternating:

  a  the grid: ops.MeshIndex (build: rows, count, one read of the entry count, fill) + cast_rays, default cell
  b  ops.cast_rays_all, the all-triangles kernel (on a ray subset where all rays would take seconds: `scaled`)
  c  utils_geometry.cast_rays_torch on the device, chunked torch ops (always on a ray subset: `scaled`)

Workloads: 640 x 480 pin-hole rays (90 degrees) from inside a furnished 8 x 6 x 3 m room whose surface is the HIP marching
cubes of its analytic signed distance at rising resolution: about 10^4, 10^5 and 10^6 triangles, no files needed.

Times are host wall clock between two device synchronisations, median (min .. max) over --repeats alternating repeats
after --warmup (five for a route whose run takes more than 0.3 s).  Also recorded: a == b bit for bit on the subset; list entries per triangle; cells visited and triangles
offered per ray; the sweep of MESH_CELL_EDGES behind the default cell; small problems on either side of MESH_ALL_BELOW;
the build of a mixed mesh (twelve wall-sized triangles added to the 10^5 mesh) at a 4 cm cell; and the rays in row-major
order against 8 x 8 pixel tiles per wavefront.

    python tools/bench_cast_rays.py [--out profiles/cast_rays.json]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOM = np.array([[0.0, 8.0], [0.0, 6.0], [0.0, 3.0]])
FURNITURE = [((1.0, 3.5, 0.0), (2.2, 4.5, 0.8)), ((5.0, 1.0, 0.0), (6.5, 1.8, 1.1)), ((3.5, 4.8, 0.0), (4.1, 5.4, 2.0))]


def room_mesh(h, dev):
    """marching cubes of the room's analytic distance (positive in free space) sampled every h metres -> (V, T) on dev"""
    from miso_amd import ops
    lo = torch.tensor(ROOM[:, 0] - 0.25, device=dev, dtype=torch.float32)
    n = [int(math.ceil((ROOM[a, 1] - ROOM[a, 0] + 0.5) / h)) + 1 for a in range(3)]
    ax = [lo[a] + h * torch.arange(n[a], device=dev, dtype=torch.float32) for a in range(3)]
    X, Y, Z = torch.meshgrid(*ax, indexing="ij")
    P = torch.stack([X, Y, Z], dim=-1)
    rlo, rhi = (torch.tensor(ROOM[:, k], device=dev, dtype=torch.float32) for k in (0, 1))
    sdf = torch.minimum(P - rlo, rhi - P).amin(dim=-1)
    for blo, bhi in FURNITURE:
        q = torch.maximum(torch.tensor(blo, device=dev) - P, P - torch.tensor(bhi, device=dev))
        sdf = torch.minimum(sdf, q.clamp(min=0).norm(dim=-1) + q.amax(dim=-1).clamp(max=0))
    sdf = sdf + 0.02 * torch.sin(3.1 * X) * torch.sin(2.7 * Y) * torch.sin(3.3 * Z)      # no face lies in a grid plane
    verts, faces = ops.marching_cubes(sdf.contiguous(), 0.0)
    return (verts * h + lo).contiguous(), faces.contiguous()


def camera_rays(dev, tiles=False):
    from miso_amd.grid_opt.utils.utils_sample import pinhole_rays_lookat
    eye = torch.tensor([2.0, 2.5, 1.4])
    rays = pinhole_rays_lookat(90.0, eye + torch.tensor([0.94, 0.34, -0.05]), eye, torch.tensor([0.0, 0.0, -1.0]), 640, 480, device=dev)
    if tiles:                                                 # 8 x 8 pixel tiles, a tile per wavefront
        r, c = torch.meshgrid(torch.arange(480, device=dev), torch.arange(640, device=dev), indexing="ij")
        key = ((r // 8) * 80 + c // 8) * 64 + (r % 8) * 8 + c % 8
        rays = rays[torch.argsort(key.reshape(-1))]
    return rays[:, :3].contiguous(), rays[:, 3:].contiguous()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "repeats": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cast_rays.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="0.2,0.063,0.02")
    args = ap.parse_args()
    from miso_amd import ops
    from miso_amd.grid_opt.utils.utils_geometry import cast_rays_torch
    dev = torch.device("cuda:0")
    O, D = camera_rays(dev)
    n = O.shape[0]
    rec = {"rays": n, "device": torch.cuda.get_device_name(0), "MESH_CELL_EDGES": ops.MESH_CELL_EDGES, "workloads": {}}
    meshes = {}
    for h in [float(x) for x in args.sizes.split(",")]:
        V, T = room_mesh(h, dev)
        nt = int(T.shape[0])
        meshes[h] = (V, T)
        sub_all = min(n, max(4096, int(2e10 // nt) // 256 * 256))      # the all-triangles route: at most 2e10 tests a run
        sub_torch = min(n, 4096)
        chunk = max(1, min(4096, (1 << 22) // nt))
        pick = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        Oa, Da = O[pick[:sub_all]].contiguous(), D[pick[:sub_all]].contiguous()
        Ot, Dt = O[pick[:sub_torch]].contiguous(), D[pick[:sub_torch]].contiguous()
        routes = {"build": lambda: ops.MeshIndex(V, T), "grid": None, "all": lambda: ops.cast_rays_all(Oa, Da, V, T),
                  "torch": lambda: cast_rays_torch(Ot, Dt, V, T, chunk=chunk)}
        ix = ops.MeshIndex(V, T)
        routes["grid"] = lambda: ix.cast_rays(O, D)
        times = {k: [] for k in routes}
        for it in range(args.warmup + args.repeats):
            for k, fn in routes.items():
                if len(times[k]) >= 5 and np.median(times[k]) > 300.0:
                    continue                                  # a route that takes a third of a second: five repeats
                ms, _ = timed(fn)
                if it >= args.warmup:
                    times[k].append(ms)
        walk = torch.zeros(3, dtype=torch.int64, device=dev)
        tg, ig = ix.cast_rays(O, D, stats=walk)
        ta, ia = ops.cast_rays_all(Oa, Da, V, T)
        tt, it_ = cast_rays_torch(Ot, Dt, V, T, chunk=chunk)
        sel = pick[:sub_all]
        w = {"triangles": nt, "vertices": int(V.shape[0]), "voxel_m": h, "index": ix.stats(),
             "routes": {k: summary(v) for k, v in times.items()},
             "all_rays": sub_all, "all_scaled_to_full_ms": float(np.median(times["all"])) * n / sub_all,
             "torch_rays": sub_torch, "torch_scaled_to_full_ms": float(np.median(times["torch"])) * n / sub_torch,
             "grid_equals_all_bit_for_bit": bool(torch.equal(tg[sel].view(torch.int32), ta.view(torch.int32)) and torch.equal(ig[sel], ia)),
             "torch_picks_the_same_triangle": float((it_ == ig[pick[:sub_torch]]).float().mean()),
             "hit_fraction": float((ig >= 0).float().mean()),
             "cells_per_ray": float(walk[0]) / n, "triangles_offered_per_ray": float(walk[1]) / n, "rays_from_all_rows": int(walk[2])}
        # rays in 8 x 8 pixel tiles per wavefront instead of image rows
        Ox, Dx = camera_rays(dev, tiles=True)
        row_ms, tile_ms = [], []
        for it in range(args.warmup + args.repeats):
            a, _ = timed(lambda: ix.cast_rays(O, D))
            b, _ = timed(lambda: ix.cast_rays(Ox, Dx))
            if it >= args.warmup:
                row_ms.append(a); tile_ms.append(b)
        w["ray_order"] = {"row_major": summary(row_ms), "tiles_8x8": summary(tile_ms)}
        # the cell behind the default: MESH_CELL_EDGES x the edge estimate
        edge = ops.mesh_default_cell(ix.bound_min, ix.bound_max, nt) / ops.MESH_CELL_EDGES
        sweep = {}
        for factor in (0.5, 1.0, 2.0, 4.0, 8.0):
            b_ms, c_ms = [], []
            for it in range(1 + 5):
                ms, jx = timed(lambda: ops.MeshIndex(V, T, cell=factor * edge))
                ms2, _ = timed(lambda: jx.cast_rays(O, D))
                if it:
                    b_ms.append(ms); c_ms.append(ms2)
            sweep[str(factor)] = {"cell": jx.cell, "entries_per_triangle": jx.stats()["entries_per_triangle"], "cells": jx.stats()["cells"],
                                  "build_ms": float(np.median(b_ms)), "cast_ms": float(np.median(c_ms))}
            del jx
        w["cell_sweep"] = sweep
        rec["workloads"][f"{nt}"] = w
        print(json.dumps({nt: w}), flush=True)
    # a mixed mesh: twelve wall-sized triangles beside 10^5 small ones, at a 4 cm cell (the count and the fill each
    # visit every box cell of every triangle; a wavefront per triangle, its lanes striding over the box)
    from miso_amd.grid_opt.utils import utils_sdf
    hs = sorted(meshes)
    V, T = meshes[hs[len(hs) // 2]]
    box = utils_sdf.box_mesh(np.array([[0.1, 7.9], [0.1, 5.9], [0.1, 2.9]]))
    slant = np.array([[0.1, 0.1, 0.1], [7.9, 0.1, 2.9], [7.9, 5.9, 2.9], [0.1, 5.9, 0.1]])          # the 8 x 6 x 3 m slanted quad
    Vb = torch.cat([V, torch.tensor(box.vertices, dtype=torch.float32, device=dev), torch.tensor(slant, dtype=torch.float32, device=dev)])
    nv = int(V.shape[0])
    Tb = torch.cat([T, torch.tensor(box.triangles, device=dev) + nv, torch.tensor([[0, 1, 2], [0, 2, 3]], device=dev) + nv + 8])
    mix = {}
    for name, (vv, tt_) in (("small_only", (V, T)), ("with_14_huge", (Vb, Tb))):
        ms = []
        for it in range(1 + 5):
            m, jx = timed(lambda: ops.MeshIndex(vv, tt_, cell=0.04))
            if it:
                ms.append(m)
        mix[name] = {"triangles": int(tt_.shape[0]), "build": summary(ms), "index": jx.stats()}
    rec["mixed_build_at_4cm"] = mix
    print(json.dumps({"mixed": mix}), flush=True)
    # either side of the route threshold: the all-triangles kernel against build + grid cast
    V, T = meshes[hs[-1]] if len(hs) == 1 else meshes[max(hs)]
    cross = []
    g = torch.Generator(device=dev).manual_seed(2)
    for nt in (12, 128, 1024, 8192):
        Ts = T[torch.randperm(T.shape[0], device=dev, generator=g)[:nt]].contiguous()
        for nr in (256, 4096, 65536):
            a_ms, g_ms = [], []
            for it in range(1 + 7):
                a, _ = timed(lambda: ops.cast_rays_all(O[:nr], D[:nr], V, Ts))
                b, _ = timed(lambda: ops.MeshIndex(V, Ts).cast_rays(O[:nr], D[:nr]))
                if it:
                    a_ms.append(a); g_ms.append(b)
            cross.append({"triangles": nt, "rays": nr, "all_ms": float(np.median(a_ms)),
                          "build_and_grid_ms": float(np.median(g_ms))})
    rec["route_threshold"] = {"MESH_ALL_BELOW": ops.MESH_ALL_BELOW, "cases": cross}
    print(json.dumps({"threshold": cross}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
