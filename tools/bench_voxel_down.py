"""Voxel down-sampling of one dataset batch, three routes on the same seeded tables, alternating:

  a  the HIP operator: ops.voxel_down_sample on the live rows + RayBatch.select (the padded batch; nothing read back)
     a_index: ops.voxel_down_sample alone
  b  the torch mirror fed CUDA tensors (utils_geometry.voxel_down_sample_torch_ops: the only device route before the
     operator; a device unique and a .max() read-back inside) + the six indexed gathers
     b_index: the mirror alone
  c  the reference's protocol (grid_opt/datasets/sdf_rgbd.py:460-470): coords.cpu(), the mirror on the host, the index
     array back to the device, six indexed gathers there

Tables: rows = keyframes x 5 000 rays x 7 samples for 1, 10 and 100 keyframes (what the ScanNet demo's mapping set
produces per batch), coordinates uniform in an 8 x 5 x 3 m room, voxel sizes 0.01 (mapping set) and 0.05 (tracking set).
Times are host wall clock between two device synchronisations (route c works on the host).

    python tools/bench_voxel_down.py [--repeats 20] [--warmup 2] [--out profiles/voxel_down.json]

Prints one JSON line; per (rows, voxel size) and route the median and the range (min .. max) in ms, whether a and c select
the same indices, and how many indices are selected by only one of a and b (the mirror on the GPU divides by a
reciprocal multiply, so it is not the reference's selection)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LO, HI = (-4.0, -2.5, -0.2), (4.0, 2.5, 2.8)
RAYS, S = 5000, 7


def table(rows, dev, seed):
    from miso_amd import ops
    g = torch.Generator().manual_seed(seed)
    lo, hi = torch.tensor(LO), torch.tensor(HI)
    b = ops.RayBatch(rows // S, S, dev)
    b.coords_frame.copy_(torch.rand(rows, 3, generator=g) * (hi - lo) + lo)
    b.sample_frame_ids.copy_(torch.randint(0, max(rows // (RAYS * S), 1), (rows,), generator=g))
    b.aux.copy_(torch.rand(rows, 4, generator=g))
    b.counts[2] = rows
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, nargs="*", default=[RAYS * S, 10 * RAYS * S, 100 * RAYS * S])
    ap.add_argument("--voxel_sizes", type=float, nargs="*", default=[0.01, 0.05])
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from miso_amd import _lib, ops
    from miso_amd.grid_opt.utils.utils_geometry import voxel_down_sample_torch_ops as mirror
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    dev = "cuda:0"
    results = []
    for rows in args.rows:
        b = table(rows, dev, seed=rows)
        cols = [b.coords_frame, b.sample_frame_ids[:, None], b.aux[:, 3:4].contiguous(), b.aux[:, 0:1].contiguous(),
                b.aux[:, 1:2].contiguous() > 0, b.aux[:, 2:3].contiguous()]          # the reference's six tensors
        out_batch = ops.RayBatch(rows // S, S, dev)
        sel = (torch.empty(rows, device=dev, dtype=torch.int64), torch.empty(1, device=dev, dtype=torch.int32))
        for v in args.voxel_sizes:
            def a_index():
                return ops.voxel_down_sample(b.coords_frame, v, n_live=b.live_rows, out=sel)

            def a():
                return b.select(*a_index(), out=out_batch)

            def b_index():
                return mirror(b.coords_frame, v)

            def b_route():
                idx = b_index()
                return idx, [c[idx] for c in cols]

            def c_route():
                idx = mirror(b.coords_frame.detach().cpu(), v).to(dev)
                return idx, [c[idx] for c in cols]

            routes = {"a": a, "a_index": a_index, "b": b_route, "b_index": b_index, "c": c_route}

            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3, out

            for _ in range(args.warmup):
                last = {k: timed(fn)[1] for k, fn in routes.items()}
            m = int(sel[1].item())
            idx_a, idx_b, idx_c = sel[0][:m], last["b_index"], last["c"][0]
            same = bool(idx_a.shape == idx_c.shape and torch.equal(idx_a, idx_c))
            rows_same = same and all(torch.equal(x[:m].reshape(-1), y.reshape(-1).to(x.dtype)) for x, y in zip(
                (out_batch.coords_frame, out_batch.sample_frame_ids, out_batch.aux[:, 3], out_batch.aux[:, 0],
                 out_batch.aux[:, 1] > 0, out_batch.aux[:, 2]), last["c"][1]))
            both = torch.cat((idx_a, idx_b)).unique(return_counts=True)[1]          # indices are unique within a route
            b_diff = int((both == 1).sum())
            times = {r: [] for r in routes}
            for _ in range(args.repeats):               # alternate, so that all routes see the same state of the machine
                for r, fn in routes.items():
                    times[r].append(timed(fn)[0])
            entry = {"rows": rows, "voxel_size": v, "selected": m, "a_equals_c": same, "a_rows_equal_c": bool(rows_same),
                     "b_selected": int(idx_b.shape[0]),
                     "b_indices_not_shared_with_a": b_diff}
            for r, t in times.items():
                t = np.asarray(t)
                entry[r] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max())}
            entry["a_faster_than_b_beyond_spread"] = bool(entry["a"]["max_ms"] < entry["b"]["min_ms"])
            results.append(entry)
            print(json.dumps(entry), file=sys.stderr)
    out = {"workload": "rows = keyframes x 5000 rays x 7 samples, uniform in an 8 x 5 x 3 m room; wall clock between "
                       "device synchronisations; routes alternate", "library": _lib.load().miso_version().decode(),
           "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "host_threads": torch.get_num_threads(),
           "results": results}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
