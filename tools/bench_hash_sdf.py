"""A hash GridNet's SDF queries at the Newer College bound (62 x 73 x 23 m, C = 4, decoder 8-64-64-1 / 12-64-64-1): the
one-launch route of grid.hash_fused (ops.hash_sdf_*, csrc/hash_sdf.hip) against the op-by-op route of the same net with
the switch off (ops.hash_encode + MLPNet as torch ops, autograd backwards) -- what a hash net runs without the switch.

 configs "hash19"   levels 1.0 m (62 x 73 x 23, dense-indexed) and 0.2 m (310 x 365 x 115, hashed) behind 2^19 rows
         "hash22+"  plus a 0.04 m level (1550 x 1825 x 575 vertices), all behind 2^22 rows
 batches N = 6 144 (launch-bound) and 262 144 points drawn uniformly in the bound ("uniform"), and 262 144 within 5 cm of
         twelve axis-aligned planes ("planes")
 rows    forward           net(x) under no_grad
         sdf_and_gradient  net.sdf_and_gradient(x): SDF and d sdf / d x, no table gradient
         forward_backward  net(x).backward(g) with every table taking a gradient (zero fill and float atomics included)

Before anything is timed the two routes must agree on the batch: SDF within 2e-6 max(1, max |sdf|), the level
tests/test_split_precision.py holds the split decoder to against float64.  Times are host wall clock between two device
synchronisations around --inner back-to-back calls, per call; median (min .. max) over --repeats repeats, the two routes
alternating inside a repeat, after a warm-up of every row on every shape.

    python tools/bench_hash_sdf.py [--out profiles/hash_sdf.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOUND = [[0.0, 62.0], [0.0, 73.0], [0.0, 23.0]]
CONFIGS = {"hash19": (2, 19), "hash22+": (3, 22)}      # levels (1.0 m, then a fifth of it each), log2 of the table


def model_cfg(levels, log2, fused):
    return {"name": "grid_net", "spatial_dim": 3,
            "decoder": {"type": "mlp", "hidden_dim": 64, "hidden_layers": 1, "out_dim": 1, "pos_invariant": True, "fix": True,
                        "pretrained_model": None},
            "grid": {"type": "hash", "log2_hashmap_size": log2, "hash_fused": fused, "feature_dim": 4, "init_stddev": 0.1,
                     "bound": BOUND, "base_cell_size": 1.0, "per_level_scale": 5.0, "n_levels": levels},
            "pose": {"optimize": False, "num_poses": 1}}


def draw(n, kind, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    b = torch.tensor(BOUND, device=dev)
    x = b[:, 0] + (b[:, 1] - b[:, 0]) * torch.rand(n, 3, generator=g, device=dev)
    if kind == "planes":
        axis = torch.randint(0, 3, (n,), generator=g, device=dev)
        plane = torch.randint(1, 5, (n,), generator=g, device=dev).float() / 5          # four planes per axis
        pos = b[axis, 0] + (b[axis, 1] - b[axis, 0]) * plane + 0.05 * (2 * torch.rand(n, generator=g, device=dev) - 1)
        x[torch.arange(n, device=dev), axis] = pos
    return x.contiguous()


def timed(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def spread(t):
    t = np.asarray(t)
    return {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()), "repeats": int(len(t))}


def rows_of(net, x, g):
    def forward():
        with torch.no_grad():
            return net(x)

    def forward_backward():
        for p in net.params_for_features():
            p.grad = None
        net(x).backward(g)

    return {"forward": forward, "sdf_and_gradient": lambda: net.sdf_and_gradient(x), "forward_backward": forward_backward}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back calls per timed window")
    ap.add_argument("--configs", nargs="*", default=list(CONFIGS))
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from miso_amd import _lib
    from miso_amd.grid_opt.models.grid_net import GridNet
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    dev = "cuda:0"
    results = []
    for cfg in args.configs:
        levels, log2 = CONFIGS[cfg]
        torch.manual_seed(1)
        nets = {"fused": GridNet(model_cfg(levels, log2, True), device=dev).to(dev)}
        nets["op_by_op"] = GridNet(model_cfg(levels, log2, False), device=dev).to(dev)
        nets["op_by_op"].load_state_dict(nets["fused"].state_dict())
        for net in nets.values():
            net.unlock_feature()
        assert nets["fused"]._fused_hash_decoder() is not None and nets["op_by_op"]._fused_hash_decoder() is None
        batches = [("uniform", 6144), ("uniform", 262144), ("planes", 262144)]
        entries = []
        for kind, n in batches:                  # agreement and warm-up of every row on every shape first
            x = draw(n, kind, dev, seed=n)
            g = torch.randn(n, 1, device=dev, generator=torch.Generator(device=dev).manual_seed(n + 1))
            fns = {route: rows_of(net, x, g) for route, net in nets.items()}
            a, b = fns["fused"]["forward"](), fns["op_by_op"]["forward"]()
            diff, scale = float((a - b).abs().max()), max(1.0, float(b.abs().max()))
            assert diff <= 2e-6 * scale, f"{cfg} {kind} {n}: the routes differ by {diff:.3e} at scale {scale:.3e}"
            (sa, ga), (sb, gb) = fns["fused"]["sdf_and_gradient"](), fns["op_by_op"]["sdf_and_gradient"]()
            for route in fns:
                fns[route]["forward_backward"]()
            gt = [[p.grad.clone() for p in net.params_for_features()] for net in nets.values()]
            entry = {"config": cfg, "dims": [list(f.dims) for f in nets["fused"].features], "log2": log2, "batch": kind, "n": n,
                     "table_MB": sum(f.feature.numel() for f in nets["fused"].features) * 4 / 1e6,
                     "max_abs_difference_fused_op_by_op": {
                         "sdf": diff, "sdf_scale": float(b.abs().max()),
                         "grad_x": float((ga - gb).abs().max()), "grad_x_scale": float(gb.abs().max()),
                         "grad_t": float(max((p - q).abs().max() for p, q in zip(*gt))),
                         "grad_t_scale": float(max(q.abs().max() for q in gt[1]))}}
            entries.append((entry, fns))
        for entry, fns in entries:
            times = {(route, row): [] for route in fns for row in fns[route]}
            for _ in range(args.repeats):        # alternate: both routes see the same state of the machine
                for row in fns["fused"]:
                    for route in fns:
                        times[(route, row)].append(timed(fns[route][row], args.inner))
            for (route, row), t in times.items():
                entry[f"{route}_{row}"] = spread(t)
            for row in fns["fused"]:
                f, o = entry[f"fused_{row}"], entry[f"op_by_op_{row}"]
                entry[f"ratio_op_by_op_over_fused_{row}"] = o["median_ms"] / f["median_ms"]
                entry[f"slowest_fused_beats_fastest_op_by_op_{row}"] = bool(f["max_ms"] < o["min_ms"])
            print(json.dumps(entry), file=sys.stderr)
            results.append(entry)
        del nets, entries
        torch.cuda.empty_cache()
    out = {"workload": "SDF queries of a hash GridNet at the Newer College bound, C = 4, decoder F-64-64-1: grid.hash_fused "
                       "against the op-by-op route of the same process; wall clock between device synchronisations around "
                       "`inner` back-to-back calls, per call; the routes alternate inside a repeat",
           "library": _lib.load().miso_version().decode(), "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "inner": args.inner,
           "not_measured": ["per-kernel times", "hardware counters", "C = 8"],
           "results": results}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
