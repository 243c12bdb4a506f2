"""Sphere tracing through the atlas: the one-launch kernel (miso_atlas_sphere_trace) against the Python loop of this
same commit, both through utils_sdf.sphere_tracing -- the model object takes the fused path, a lambda around it the loop.

Scene: the analytic room of tools/demo_synthetic.py (ROOM, moved into the overlap of the submaps) baked into the grids of
the 8 ScanNet-shaped submaps of bench.py the way tests/sphere_trace_cases.py bakes its scene: the signed distance at every
voxel centre, value / n_levels in channel 0 of each level, behind a pass-through decoder.  Workload: 640 x 480 rays from
each of two camera poses, max_iters 100, epsilon 1e-5 (the defaults of sphere_tracing).

    python tools/bench_sphere_trace.py [--repeats 20] [--out profiles/sphere_trace.json]

Prints one JSON line: median and spread (min .. max) of both paths in ms, rays/s, field evaluations/s (sum(steps) + N per
trace), and the live-lane share sum(steps) / (64 * sum over wavefronts of the wavefront's max steps)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOM = np.array([[0.0, 8.0], [0.0, 6.0], [0.0, 3.0]])      # tools/demo_synthetic.py
OFFSET = np.array([11.0, -3.0, 1.0])                        # the room inside the atlas: x 11..19, y -3..3, z 1..4
H, W = 480, 640


def room_sdf(p):
    """(N,3) world points -> (N,) distance to the nearest wall, positive inside the room."""
    lo = torch.tensor(ROOM[:, 0] + OFFSET, device=p.device, dtype=p.dtype)
    hi = torch.tensor(ROOM[:, 1] + OFFSET, device=p.device, dtype=p.dtype)
    return torch.minimum(p - lo, hi - p).min(dim=-1).values


def bake(atlas):
    """the room into every submap's grids, the pass-through decoder into every submap"""
    with torch.no_grad():
        for s in range(atlas.num_submaps):
            net = atlas.get_submap(s)
            R, t = atlas.updated_submap_pose(s)
            L = len(net.features)
            for g in net.features:
                f = g.feature
                _, C, Z, Y, X = f.shape
                world = g.vertex_positions() @ R.T + t.reshape(1, 3)
                f.zero_()
                f[0, 0].copy_((room_sdf(world) / L).reshape(Z, Y, X))
            lin = net.decoder.linears()
            F_, C = lin[0].weight.shape[1], net.features[0].feature.shape[1]
            for m in lin:
                m.weight.zero_()
                m.bias.zero_()
            lin[0].weight[0, 0:F_:C] = 1.0          # h0 = relu(+sum), h1 = relu(-sum)
            lin[0].weight[1, 0:F_:C] = -1.0
            lin[1].weight[0, 0] = lin[1].weight[1, 1] = 1.0
            lin[2].weight[0, 0], lin[2].weight[0, 1] = 1.0, -1.0
    return atlas


def camera_rays(eye, look_at, dev):
    eye = np.asarray(eye, dtype=np.float64)
    fwd = np.asarray(look_at, dtype=np.float64) - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))        # z up, as in the demo
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack((right, down, fwd), axis=1)
    r, c = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dc = np.stack(((c - (W - 1) / 2) / (0.9 * W), (r - (H - 1) / 2) / (0.9 * W), np.ones_like(c)), -1).reshape(-1, 3)
    d = torch.tensor(dc @ R.T, dtype=torch.float32, device=dev)
    o = torch.tensor(eye, dtype=torch.float32, device=dev).expand_as(d).contiguous()
    return o, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import bench
    import miso_amd.grid_opt.utils.utils_sdf as US
    from miso_amd import _lib
    dev = "cuda:0"
    atlas = bake(bench.scannet_atlas(dev, 8))
    centre = ROOM.mean(axis=1) + OFFSET
    poses = [(centre + [-2.0, 0.5, 0.0], centre + [4.0, -1.0, -0.4]), (centre + [2.5, -1.5, 0.3], centre + [-4.0, 3.0, -1.0])]
    rays = [camera_rays(e, l, dev) for e, l in poses]
    o, d = torch.cat([r[0] for r in rays]), torch.cat([r[1] for r in rays])
    n = o.shape[0]
    kw = dict(max_dist=12.0)
    paths = {"fused": atlas, "loop": lambda p: atlas(p)}

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
        same = bool(torch.equal(res["fused"][0], res["loop"][0]) and torch.equal(res["fused"][1], res["loop"][1]))
        times = {k: [] for k in paths}
        for _ in range(args.repeats):                 # alternate, so that both see the same state of the machine
            for k, q in paths.items():
                times[k].append(timed(q)[0])
        _, mask, extras = atlas.sphere_trace(o, d, want_steps=True, **kw)
    steps = extras["steps"].to(torch.int64)
    pad = (-n) % 64
    per_wave = torch.cat((steps, steps.new_zeros(pad))).reshape(-1, 64)
    evals = int(steps.sum()) + n
    out = {"workload": f"{len(poses)} x {W}x{H} rays, 8 ScanNet-shaped submaps, max_iters 100, epsilon 1e-5, max_dist 12",
           "library": _lib.load().miso_version().decode(), "device": torch.cuda.get_device_name(0), "rays": n,
           "repeats": args.repeats, "fused_equals_loop": same, "hit_share": float(mask.float().mean()),
           "field_evaluations": evals, "mean_steps": float(steps.float().mean()), "max_steps": int(steps.max()),
           "live_lane_share": float(steps.sum()) / float(64 * per_wave.max(dim=1).values.sum())}
    for k, t in times.items():
        t = np.asarray(t)
        out[k] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()),
                  "rays_per_s": n / (np.median(t) * 1e-3), "evaluations_per_s": evals / (np.median(t) * 1e-3)}
    out["speedup_median"] = out["loop"]["median_ms"] / out["fused"]["median_ms"]
    # faster by more than the run-to-run spread of this run: the slowest fused repeat against the fastest loop repeat
    out["fused_faster_beyond_spread"] = bool(out["fused"]["max_ms"] < out["loop"]["min_ms"])
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
