"""Distance from points to a mesh, the routes on the same queries, alternating:

  build      ops.MeshIndex + prepare_distance(): the index and its coarse level (two counts, two host reads, two fills)
  closest    MeshIndex.closest: the shell walk, fine index then coarse
  signed     MeshIndex.signed_distance: closest + contains (three crossing counts per point)
  all        ops.closest_all, the all-triangles kernel (on a subset where all queries would take seconds: `scaled`)
  torch      utils_geometry.closest_on_mesh_torch on the device, chunked torch ops (always on a subset: `scaled`)
  fine_only  closest(far=False): the fine shells to their end, on the two smaller meshes (why the coarse level exists)

Workloads: the furnished 8 x 6 x 3 m room of tools/bench_cast_rays.py at about 10^4, 10^5 and 10^6 triangles; queries are
Sdf3D's own mix at 2^19 points: 3/4 surface samples moved by a Gaussian of 0.1 m, 1/4 uniform in the box + 0.5 m.

Times are host wall clock between two device synchronisations, median (min .. max) over --repeats alternating repeats
after --warmup (five for a route whose run takes more than 0.3 s).  Also recorded: closest == all bit for bit on the
subset; the share of queries that went to the coarse index and that were answered from all rows; cells and triangles per
query; and at the largest mesh the sweep of the coarse level's cell factor and of the fine shells walked first.

    python tools/bench_mesh_sdf.py [--out profiles/mesh_sdf.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_cast_rays import ROOM, room_mesh, summary, timed  # noqa: E402


def queries(V, T, n, dev):
    from miso_amd.grid_opt.utils.utils_eval import sample_surface
    g = torch.Generator(device=dev).manual_seed(3)
    near = sample_surface(V, T, n * 3 // 4, g)[0].float()
    near = near + 0.1 * torch.randn(near.shape, device=dev, generator=g)
    lo, hi = (torch.tensor(ROOM[:, k], device=dev, dtype=torch.float32) + s for k, s in ((0, -0.5), (1, 0.5)))
    uni = lo + (hi - lo) * torch.rand((n - near.shape[0], 3), device=dev, generator=g)
    return torch.cat([near, uni])[torch.randperm(n, device=dev, generator=g)].contiguous()


def run_routes(routes, warmup, repeats):
    times = {k: [] for k in routes}
    for it in range(warmup + repeats):
        for k, fn in routes.items():
            if len(times[k]) >= 5 and np.median(times[k]) > 300.0:
                continue                                      # a route that takes a third of a second: five repeats
            ms, _ = timed(fn)
            if it >= warmup:
                times[k].append(ms)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_sdf.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="0.2,0.063,0.02")
    ap.add_argument("--points", type=int, default=2 ** 19)
    args = ap.parse_args()
    from miso_amd import ops
    from miso_amd.grid_opt.utils.utils_geometry import closest_on_mesh_torch
    dev = torch.device("cuda:0")
    n = args.points
    rec = {"points": n, "device": torch.cuda.get_device_name(0), "MESH_FAR_FACTOR": ops.MESH_FAR_FACTOR,
           "MESH_FAR_RINGS": ops.MESH_FAR_RINGS, "workloads": {}}
    sizes = [float(x) for x in args.sizes.split(",")]
    for h in sizes:
        V, T = room_mesh(h, dev)
        nt = int(T.shape[0])
        P = queries(V, T, n, dev)
        sub_all = min(n, max(4096, int(1e10 // nt) // 256 * 256))       # the all-triangles route: at most 1e10 pairs a run
        sub_torch = min(n, 4096, max(256, (1 << 30) // nt // 256 * 256))
        chunk = max(1, min(1024, (1 << 21) // nt))
        Pa, Pt = P[:sub_all].contiguous(), P[:sub_torch].contiguous()
        ix = ops.MeshIndex(V, T).prepare_distance()
        routes = {"build": lambda: ops.MeshIndex(V, T).prepare_distance(), "closest": lambda: ix.closest(P),
                  "signed": lambda: ix.signed_distance(P), "all": lambda: ops.closest_all(Pa, V, T),
                  "torch": lambda: closest_on_mesh_torch(Pt, V, T, chunk=chunk)}
        times = run_routes(routes, args.warmup, args.repeats)
        stats = torch.zeros(5, dtype=torch.int64, device=dev)
        d2, tri = ix.closest(P, stats=stats)
        da, ta = ops.closest_all(Pa, V, T)
        dt, tt, _ = closest_on_mesh_torch(Pt, V, T, chunk=chunk)
        st = [int(x) for x in stats.cpu()]
        w = {"triangles": nt, "vertices": int(V.shape[0]), "voxel_m": h, "index": ix.stats(),
             "coarse_index": {"cell": float(ix.far[0].cell), "dims": [int(x) for x in ix.far[0].dims], "entries": int(ix.far[1])},
             "routes": {k: summary(v) for k, v in times.items()},
             "all_points": sub_all, "all_scaled_to_full_ms": float(np.median(times["all"])) * n / sub_all,
             "torch_points": sub_torch, "torch_scaled_to_full_ms": float(np.median(times["torch"])) * n / sub_torch,
             "closest_equals_all_bit_for_bit": bool(torch.equal(d2[:sub_all].view(torch.int32), da.view(torch.int32)) and
                                                    torch.equal(tri[:sub_all], ta)),
             "torch_picks_the_same_triangle": float((tt == tri[:sub_torch]).float().mean()),
             "inside_fraction": float(ix.contains(P).float().mean()),
             "fine_cells_per_query": st[0] / n, "coarse_cells_per_query": st[1] / n, "triangles_offered_per_query": st[2] / n,
             "went_coarse_share": st[3] / n, "from_all_rows": st[4]}
        if h != min(sizes) or len(sizes) == 1:
            ms = [timed(lambda: ix.closest(P, far=False))[0] for _ in range(4)][1:]
            ix.closest(P, stats=stats, far=False)
            w["fine_only"] = dict(summary(ms), fine_cells_per_query=int(stats.cpu()[0]) / n)
        if h == min(sizes):
            sweep = []
            for factor in (4, 8, 16):
                for rings in (1, 2, 3, 5):
                    ix.prepare_distance(factor, rings)
                    ms = [timed(lambda: ix.closest(P))[0] for _ in range(6)][1:]
                    ix.closest(P, stats=stats)
                    s = [int(x) for x in stats.cpu()]
                    sweep.append({"factor": factor, "rings": rings, "closest_ms": float(np.median(ms)), "min_ms": float(np.min(ms)),
                                  "went_coarse_share": s[3] / n, "fine_cells_per_query": s[0] / n, "coarse_cells_per_query": s[1] / n,
                                  "triangles_offered_per_query": s[2] / n, "coarse_entries": int(ix.far[1])})
                    print(json.dumps(sweep[-1]), flush=True)
            best = min(sweep, key=lambda r: r["closest_ms"])
            w["far_sweep"] = {"cases": sweep, "fastest": {"factor": best["factor"], "rings": best["rings"]},
                              "chosen": {"factor": ops.MESH_FAR_FACTOR, "rings": ops.MESH_FAR_RINGS}}
        rec["workloads"][f"{nt}"] = w
        print(json.dumps({nt: {k: v for k, v in w.items() if k != "far_sweep"}}), flush=True)
        del ix
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
