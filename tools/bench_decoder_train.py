"""A training step with a TRAINABLE decoder: the fused route (one-kernel forward, one-kernel backward, HIP weight gradients:
csrc/decoder_wgrad.hip) against the op-by-op route such a decoder took before (grid_net._FUSED_WGRAD = False: query_feature +
utils.grid_decode under torch autograd), and the frozen-decoder step for context.

Step = GridNet.forward + L1 loss + backward + DenseAdam over the grids and the decoder, 262 144 uniform points, at
  cfg2: 3 levels of 8 features (32^3, 64^3, 128^3 cells), 64 hidden units
  nc:   the Newer College decoder shape, 2 levels of 4 features, 64 hidden units
The routes alternate run by run inside one process, after a common warm-up, so that all see the same state of the
machine.  Beside the steps: the weight-gradient launch alone and the backward launch (sdf_bwd_kernel + the grid-gradient
pull) for the same binned batch, by HIP events over back-to-back calls -- each figure is a whole operator call: the
weight-gradient kernel with its small reduce kernel; sdf_bwd_kernel with the pull that forms the grid gradients.

    python tools/bench_decoder_train.py [--runs 5] [--iters 20] [--out profiles/decoder_train.json]

Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 262144
SHAPES = {"cfg2": dict(C=8, L=3, H=64, base=2.0 / 32), "nc": dict(C=4, L=2, H=64, base=2.0 / 40)}


def model(shape, fix, dev):
    from miso_amd.grid_opt.models.grid_net import GridNet
    s = SHAPES[shape]
    cfg = {"name": "grid_net", "spatial_dim": 3,
           "decoder": {"type": "mlp", "hidden_dim": s["H"], "hidden_layers": 1, "out_dim": 1, "pos_invariant": True,
                       "fix": fix, "pretrained_model": None},
           "grid": {"type": "regular", "feature_dim": s["C"], "init_stddev": 1e-2, "bound": [[-1.0, 1.0]] * 3,
                    "base_cell_size": s["base"], "per_level_scale": 2, "n_levels": s["L"]},
           "pose": {"optimize": False, "num_poses": 1}}
    torch.manual_seed(0)
    net = GridNet(cfg, device=dev).to(dev)
    net.unlock_feature()
    return net


def events(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3      # us


def spread(t):
    t = np.asarray(t)
    return {"median_us": float(np.median(t)), "min_us": float(t.min()), "max_us": float(t.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert args.runs >= 3
    import miso_amd.grid_opt.models.grid_net as GN
    from miso_amd import _lib, ops
    from miso_amd.optim import DenseAdam
    dev = "cuda:0"
    out = {"call_alone_contains": {"wgrad": "decoder_wgrad_kernel + wgrad_reduce_kernel (ops.sdf_wgrad_raw)",
                                   "sdf_bwd": "sdf_bwd_kernel + the grid-gradient pull (ops.sdf_bwd_raw, binned, overwrite)",
                                   "how": "HIP events around back-to-back calls: device time unless the host is slower"},
           "workload": f"forward + L1 loss + backward + DenseAdam, {N} points", "library": _lib.load().miso_version().decode(),
           "device": torch.cuda.get_device_name(0), "runs": args.runs, "iters_per_run": args.iters}
    for shape in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(1)
        x = torch.rand(N, 3, device=dev, generator=gen) * 1.9 - 0.95
        target = torch.rand(N, 1, device=dev, generator=gen) * 0.2 - 0.1
        routes = {}
        for name, fix, fused in (("frozen", True, True), ("trainable_fused", False, True), ("trainable_torch", False, False)):
            net = model(shape, fix, dev)
            params = [g.feature for g in net.features] + [p for p in net.decoder.parameters() if p.requires_grad]
            opt = DenseAdam(params, lr=1e-3)

            def step(net=net, opt=opt, fused=fused):
                GN._FUSED_WGRAD = fused
                opt.zero_grad(set_to_none=True)
                loss = (net(x) - target).abs().mean()
                loss.backward()
                opt.step()
            routes[name] = step
        launches = []
        real = ops.sdf_wgrad_raw
        ops.sdf_wgrad_raw = lambda *a, **k: launches.append(1) or real(*a, **k)
        for step in routes.values():
            step()
        assert len(launches) == 1, "exactly the fused trainable route runs the weight-gradient kernel"
        ops.sdf_wgrad_raw = real
        for _ in range(args.warmup):      # past allocator growth and the clock ramp, every route alike
            for step in routes.values():
                step()
        torch.cuda.synchronize()
        times = {k: [] for k in routes}
        for _ in range(args.runs):
            for k, step in routes.items():
                times[k].append(events(step, args.iters))
        GN._FUSED_WGRAD = True
        res = {k: spread(t) for k, t in times.items()}
        res["speedup_median"] = res["trainable_torch"]["median_us"] / res["trainable_fused"]["median_us"]
        res["fused_faster_beyond_spread"] = bool(res["trainable_fused"]["max_us"] < res["trainable_torch"]["min_us"])

        # the launches alone, on the binned batch a step of this size uses
        net = model(shape, False, dev)
        feats = [g.feature.detach() for g in net.features]
        meta = net.features[0].grid_meta(net.ignore_level_)
        pack = net.decoder.decoder_pack(trainable=True)
        sb = ops.SortedBatch(N, x.device).sort(x, meta)
        _, mask = ops.sdf_fwd_raw(x, feats, meta, pack, want_mask=True, sorted_batch=sb)
        gsdf = torch.randn(N, 1, device=dev, generator=gen) / N
        grads = [torch.empty_like(f) for f in feats]
        alone = {"wgrad": lambda: ops.sdf_wgrad_raw(x, feats, meta, pack, gsdf, mask, sorted_batch=sb),
                 "sdf_bwd": lambda: ops.sdf_bwd_raw(x, feats, meta, pack, gsdf, mask, False, [True] * len(feats), grads=grads,
                                                    sorted_batch=sb, overwrite=True)}
        for fn in alone.values():
            for _ in range(args.warmup):
                fn()
        kt = {k: [] for k in alone}
        for _ in range(args.runs):
            for k, fn in alone.items():
                kt[k].append(events(fn, args.iters))
        res["wgrad_call_alone"] = spread(kt["wgrad"])
        res["sdf_bwd_call_alone"] = spread(kt["sdf_bwd"])
        out[shape] = res
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
