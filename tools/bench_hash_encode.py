"""ops.hash_encode at the Newer College bound (62 x 73 x 23 m, C = 4): forward, table gradient and x gradient, against
what a user has without it.

 levels  "dense"      1.0 m (62 x 73 x 23) and 0.2 m (310 x 365 x 115: 52 M floats) as dense FeatureGrid levels: ops.encode
         "hash19"     the same two levels behind 2^19 rows (the coarse one dense-indexed, the fine one hashed: 8 MB)
         "hash22"     ... behind 2^22 rows (64 MB)
         "hash22+"    plus a 0.04 m level (1550 x 1825 x 575 vertices: 24 GiB dense, cannot exist) behind 2^22 rows
 batches N = 6 144 and 262 144 points, drawn uniformly in the bound ("uniform") and within 5 cm of twelve axis-aligned
         planes ("planes": samples hugging surfaces share cells, hence rows)
 routes  hip    ops.hash_encode_fwd_raw / hash_encode_bwd_raw (csrc/hash_encode.hip)
         dense  ops.encode_fwd_raw / encode_bwd_raw on the dense levels ("dense" only; the library's own choice of path:
                from 16 384 points the grid gradient is binned and pulled, not scattered)
         torch  the same hash encode written as torch ops on the device: index arithmetic in int64, gather, index_add_
                (hash_encode_torch below) -- what a user can do today
 ops     fwd; grad_t (table gradients only, zero-filled gradient buffers included); grad_x (x gradient only)

Times are host wall clock between two device synchronisations around --inner back-to-back calls, per call; median
(min .. max) over --repeats repeats, the routes alternating inside a repeat, after a warm-up of every route and shape.
Beside each hip time: the bytes the op must move (8 corners x 4 C bytes per level and point, gathered or added) over the
time, to read against the gather and float-atomic rates of the hardware (the "rates" entry of the output).

    python tools/bench_hash_encode.py [--out profiles/hash_encode.json]"""
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
C = 4
PRIME_Y, PRIME_Z, M32 = 2654435761, 805459861, 0xFFFFFFFF


def level_dims(cell):
    return tuple(int(np.ceil((hi - lo) / cell)) for lo, hi in BOUND)


def _corners(x, bound, dims, log2):
    """per corner k: (rows (N,) int64, weight (N,), d weight / d ix (N,3)), zero weight where out of range; and d ix / d x"""
    lo, hi = bound[:, 0], bound[:, 1]
    size = torch.tensor(dims, device=x.device, dtype=x.dtype)
    ix = ((2 * (x - lo) / (hi - lo) - 1 + 1) * size - 1) / 2
    f = torch.floor(ix)
    t = ix - f
    i0 = f.long()
    rows_n, dense = (dims[0] * dims[1] * dims[2], True) if dims[0] * dims[1] * dims[2] <= 1 << log2 else (1 << log2, False)
    out = []
    for k in range(8):
        o = (k & 1, (k >> 1) & 1, k >> 2)
        c = [i0[:, a] + o[a] for a in range(3)]
        inb = torch.ones_like(c[0], dtype=torch.bool)
        for a in range(3):
            inb &= (c[a] >= 0) & (c[a] < dims[a])
        c = [torch.where(inb, v, torch.zeros_like(v)) for v in c]
        if dense:
            rows = (c[2] * dims[1] + c[1]) * dims[0] + c[0]
        else:
            rows = (c[0] ^ ((c[1] * PRIME_Y) & M32) ^ ((c[2] * PRIME_Z) & M32)) & (rows_n - 1)
        w1 = [t[:, a] if o[a] else 1 - t[:, a] for a in range(3)]
        sg = [1.0 if o[a] else -1.0 for a in range(3)]
        m = inb.to(x.dtype)
        w = w1[0] * w1[1] * w1[2] * m
        dw = torch.stack((sg[0] * w1[1] * w1[2] * m, sg[1] * w1[0] * w1[2] * m, sg[2] * w1[0] * w1[1] * m), 1)
        out.append((rows, w, dw))
    return out, size / (hi - lo)


def hash_encode_torch(x, tables, bound, dims, log2, gout=None, want=("fwd",)):
    """The hash encode as torch ops.  -> dict with "fwd" (N, sum C), "grad_t" [per level (rows, C)], "grad_x" (N,3)."""
    res = {}
    feats, gts, gx = [], [], torch.zeros_like(x)
    foff = 0
    for t, d in zip(tables, dims):
        corners, mult = _corners(x, bound, d, log2)
        go = None if gout is None else gout[:, foff:foff + t.shape[1]]
        if "fwd" in want:
            feats.append(sum(w[:, None] * t[rows] for rows, w, _ in corners))
        if "grad_t" in want:
            g = torch.zeros_like(t)
            for rows, w, _ in corners:
                g.index_add_(0, rows, w[:, None] * go)
            gts.append(g)
        if "grad_x" in want:
            gx = gx + mult * sum(dw * (go * t[rows]).sum(1, keepdim=True) for rows, _, dw in corners)
        foff += t.shape[1]
    if "fwd" in want:
        res["fwd"] = torch.cat(feats, 1)
    if "grad_t" in want:
        res["grad_t"] = gts
    if "grad_x" in want:
        res["grad_x"] = gx
    return res


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back calls per timed window")
    ap.add_argument("--sizes", type=int, nargs="*", default=[6144, 262144])
    ap.add_argument("--configs", nargs="*", default=["dense", "hash19", "hash22", "hash22+"])
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from miso_amd import _lib, ops
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    dev = "cuda:0"
    meta = ops.GridMeta.from_bound(BOUND)
    bound = torch.tensor(BOUND, device=dev)
    cells = {"dense": (1.0, 0.2), "hash19": (1.0, 0.2), "hash22": (1.0, 0.2), "hash22+": (1.0, 0.2, 0.04)}
    log2s = {"hash19": 19, "hash22": 22, "hash22+": 22}
    gen = torch.Generator(device=dev).manual_seed(1)
    results = []
    for cfg in args.configs:
        dims = [level_dims(c) for c in cells[cfg]]
        F = C * len(dims)
        if cfg == "dense":
            params = [(torch.randn(1, C, z, y, x, generator=gen, device=dev) * 0.1).contiguous(memory_format=torch.channels_last_3d)
                      for x, y, z in dims]
        else:
            params = [torch.randn(ops.hash_level_rows(d, log2s[cfg])[0], C, generator=gen, device=dev) * 0.1 for d in dims]
        for kind in ("uniform", "planes"):
            for n in args.sizes:
                x = draw(n, kind, dev, seed=n)
                gout = torch.randn(n, F, generator=gen, device=dev)
                none, every = [False] * len(dims), [True] * len(dims)
                if cfg == "dense":
                    routes = {("dense", "fwd"): lambda: ops.encode_fwd_raw(x, params, meta),
                              ("dense", "grad_t"): lambda: ops.encode_bwd_raw(x, params, meta, gout, False, every),
                              ("dense", "grad_x"): lambda: ops.encode_bwd_raw(x, params, meta, gout, True, none)}
                else:
                    B = log2s[cfg]
                    routes = {("hip", "fwd"): lambda: ops.hash_encode_fwd_raw(x, params, meta, dims, B),
                              ("hip", "grad_t"): lambda: ops.hash_encode_bwd_raw(x, params, meta, dims, B, gout, False, every),
                              ("hip", "grad_x"): lambda: ops.hash_encode_bwd_raw(x, params, meta, dims, B, gout, True, none),
                              ("torch", "fwd"): lambda: hash_encode_torch(x, params, bound, dims, B),
                              ("torch", "grad_t"): lambda: hash_encode_torch(x, params, bound, dims, B, gout, ("grad_t",)),
                              ("torch", "grad_x"): lambda: hash_encode_torch(x, params, bound, dims, B, gout, ("grad_x",))}
                entry = {"config": cfg, "dims": [list(d) for d in dims], "log2": log2s.get(cfg), "batch": kind, "n": n,
                         "parameter_MB": sum(p.numel() for p in params) * 4 / 1e6}
                if cfg != "dense":                      # the two formulations agree (fp32 reordering apart) before they are timed
                    B = log2s[cfg]
                    a, b = routes[("hip", "fwd")](), routes[("torch", "fwd")]()["fwd"]
                    ga, gb = routes[("hip", "grad_t")]()[1], routes[("torch", "grad_t")]()["grad_t"]
                    xa, xb = routes[("hip", "grad_x")]()[0], routes[("torch", "grad_x")]()["grad_x"]
                    entry["max_abs_difference_hip_torch"] = {
                        "fwd": float((a - b).abs().max()), "grad_t": float(max((p - q).abs().max() for p, q in zip(ga, gb))),
                        "grad_x": float((xa - xb).abs().max()), "fwd_scale": float(b.abs().max()),
                        "grad_t_scale": float(max(q.abs().max() for q in gb)), "grad_x_scale": float(xb.abs().max())}
                for fn in routes.values():              # warm-up of every route on this shape
                    fn()
                times = {r: [] for r in routes}
                for _ in range(args.repeats):           # alternate: every route sees the same state of the machine
                    for r, fn in routes.items():
                        times[r].append(timed(fn, args.inner))
                moved = n * 8 * C * 4 * len(dims)       # bytes gathered (fwd, grad_x) or added (grad_t)
                for (route, op), t in times.items():
                    s = spread(t)
                    if route != "torch":
                        s["bytes"] = moved
                        s["GB_per_s_at_median"] = moved / (s["median_ms"] * 1e-3) / 1e9
                    entry[f"{route}_{op}"] = s
                if cfg != "dense":
                    for op in ("fwd", "grad_t", "grad_x"):
                        h, t = entry[f"hip_{op}"], entry[f"torch_{op}"]
                        entry[f"ratio_torch_over_hip_{op}"] = t["median_ms"] / h["median_ms"]
                        entry[f"slowest_hip_beats_fastest_torch_{op}"] = bool(h["max_ms"] < t["min_ms"])
                print(json.dumps(entry), file=sys.stderr)
                results.append(entry)
        del params
        torch.cuda.empty_cache()
    out = {"workload": "multi-level trilinear encode at the Newer College bound, C = 4; wall clock between device "
                       "synchronisations around `inner` back-to-back calls, per call; routes alternate inside a repeat",
           "library": _lib.load().miso_version().decode(), "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "inner": args.inner,
           "rates": {"note": "MI355X figures to read GB_per_s_at_median against",
                     "gather_infinity_cache_TB_per_s": 8.6, "gather_hbm_TB_per_s": 6.0,
                     "float_atomics_shaped_TB_per_s": 1.3, "float_atomics_64_rows_per_instruction_TB_per_s": 0.08,
                     "float_atomics_8_to_64_byte_segments": "not measured before; hip_grad_t is that measurement"},
           "results": results}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
