"""Sphere tracing through a hash GridNet: the one-launch kernel of grid.hash_fused (GridNet.sphere_trace ->
ops.hash_sphere_trace, csrc/hash_trace.hip) against the Python loop of utils_sdf.sphere_tracing over the same net's fused
forward (``lambda p: net(p)``: one ops.hash_sdf_fused launch per round, the elementwise ops and a host synchronisation
around it) -- what a hash net ran before this route existed, with the switch on.

The net is tools/bench_hash_sdf.py's "hash19": the Newer College bound (62 x 73 x 23 m), levels 1.0 m (dense-indexed) and
0.2 m (310 x 365 x 115 vertices, hashed) behind 2^19 rows, C = 4, decoder 8-64-64-1.  Scene: the analytic room of
tools/demo_synthetic.py moved inside that bound, its signed distance at the cell centres of the 1.0 m level in channel 0
behind the pass-through decoder of tests/sphere_trace_cases.py; the hashed level holds zeros in the channel the decoder
reads (its vertices share rows: it cannot hold a field per vertex without training) and random values in the others, so
its rows are gathered at every evaluation as in a trained map.  Workload: 640 x 480 pinhole rays from each of two poses
inside the room, max_iters 100, epsilon 1e-5 (the defaults of sphere_tracing).

Before anything is timed the two routes must give the same points and masks, bit for bit.  Times are device time between
two events around one call; median (min .. max) over --repeats repeats, the two routes alternating inside a repeat.

    python tools/bench_hash_trace.py [--repeats 20] [--out profiles/hash_trace.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROOM = np.array([[0.0, 8.0], [0.0, 6.0], [0.0, 3.0]])      # tools/demo_synthetic.py
OFFSET = np.array([20.0, 30.0, 5.0])                        # the room inside the bound: x 20..28, y 30..36, z 5..8
H, W = 480, 640


def room_sdf(p):
    """(N,3) points -> (N,) distance to the nearest wall, positive inside the room."""
    lo = torch.tensor(ROOM[:, 0] + OFFSET, device=p.device, dtype=p.dtype)
    hi = torch.tensor(ROOM[:, 1] + OFFSET, device=p.device, dtype=p.dtype)
    return torch.minimum(p - lo, hi - p).min(dim=-1).values


def bake(net):
    """the room into the dense-indexed level, the pass-through decoder reading channel 0 of that level"""
    with torch.no_grad():
        coarse, fine = net.features
        assert coarse.dense_indexed and not fine.dense_indexed
        gen = torch.Generator().manual_seed(2)
        for g in (coarse, fine):
            g.feature.copy_((torch.randn(g.feature.shape, generator=gen) * 0.1).to(g.feature))
            g.feature[:, 0] = 0.0
        coarse.feature[:, 0] = room_sdf(coarse.cell_centres().to(coarse.feature))
        lin = net.decoder.linears()
        for m in lin:
            m.weight.zero_()
            m.bias.zero_()
        lin[0].weight[0, 0], lin[0].weight[1, 0] = 1.0, -1.0          # h0 = relu(+v), h1 = relu(-v)
        lin[1].weight[0, 0] = lin[1].weight[1, 1] = 1.0
        lin[2].weight[0, 0], lin[2].weight[0, 1] = 1.0, -1.0
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import bench_hash_sdf
    import bench_sphere_trace
    import miso_amd.grid_opt.utils.utils_sdf as US
    from miso_amd import _lib
    from miso_amd.grid_opt.models.grid_net import GridNet
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    dev = "cuda:0"
    levels, log2 = bench_hash_sdf.CONFIGS["hash19"]
    torch.manual_seed(1)
    net = bake(GridNet(bench_hash_sdf.model_cfg(levels, log2, True), device=dev).to(dev))
    assert net._fused_hash_decoder() is not None
    centre = ROOM.mean(axis=1) + OFFSET
    poses = [(centre + [-2.0, 0.5, 0.0], centre + [4.0, -1.0, -0.4]), (centre + [2.5, -1.5, 0.3], centre + [-4.0, 3.0, -1.0])]
    rays = [bench_sphere_trace.camera_rays(e, l, dev) for e, l in poses]
    o, d = torch.cat([r[0] for r in rays]), torch.cat([r[1] for r in rays])
    n = o.shape[0]
    kw = dict(max_dist=12.0)                       # farther than the room's diagonal: no ray goes far
    paths = {"fused": net, "loop": lambda p: net(p)}

    def timed(q):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = US.sphere_tracing(q, o, d, **kw)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    with torch.no_grad():
        for _ in range(args.warmup):
            res = {k: timed(q)[1] for k, q in paths.items()}
        assert torch.equal(res["fused"][0].view(torch.int32), res["loop"][0].view(torch.int32)), "points differ"
        assert torch.equal(res["fused"][1], res["loop"][1]), "masks differ"
        times = {k: [] for k in paths}
        for _ in range(args.repeats):                 # alternate, so that both see the same state of the machine
            for k, q in paths.items():
                times[k].append(timed(q)[0])
        _, mask, extras = net.sphere_trace(o, d, want_steps=True, **kw)
    steps = extras["steps"].to(torch.int64)
    per_wave = torch.cat((steps, steps.new_zeros((-n) % 64))).reshape(-1, 64)
    evals = int(steps.sum()) + n
    out = {"workload": f"{len(poses)} x {W}x{H} rays into a hash GridNet (levels 1.0 m + 0.2 m, C = 4, 2^{log2} rows, decoder "
                       "8-64-64-1) holding an analytic room, max_iters 100, epsilon 1e-5, max_dist 12; device time between "
                       "events around one call, the routes alternating inside a repeat",
           "library": _lib.load().miso_version().decode(), "device": torch.cuda.get_device_name(0), "rays": n,
           "dims": [list(f.dims) for f in net.features], "repeats": args.repeats, "fused_equals_loop": True,
           "hit_share": float(mask.float().mean()), "field_evaluations": evals, "mean_steps": float(steps.float().mean()),
           "max_steps": int(steps.max()),
           "live_lane_share": float(steps.sum()) / float(64 * per_wave.max(dim=1).values.sum()),
           "not_measured": ["per-kernel times", "hardware counters", "C = 8", "a trained map"]}
    for k, t in times.items():
        t = np.asarray(t)
        out[k] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()),
                  "rays_per_s": n / (np.median(t) * 1e-3), "evaluations_per_s": evals / (np.median(t) * 1e-3)}
    out["speedup_median"] = out["loop"]["median_ms"] / out["fused"]["median_ms"]
    # faster by more than the run-to-run spread of this run: the slowest one-launch repeat against the fastest loop repeat
    out["slowest_fused_beats_fastest_loop"] = bool(out["fused"]["max_ms"] < out["loop"]["min_ms"])
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
