"""Pretrain a decoder on analytic scenes: one shared MLPNet, one small GridNet per scene, every step on the fused route
(one-kernel forward, one-kernel backward, HIP weight gradients: ops.sdf_fused with a trainable decoder).

The reference ships its configs with `decoder.fix: True` and a pretrained decoder that is a separate download; its own
pretraining (training/train_decoder.py:73-179) fits a shared MLP and per-scene grids to mesh SDF samples with an L2 +
free-space loss.  This tool does the same on scenes that need no files: unions of spheres and boxes above a ground plane,
sampled on the device -- near-surface samples that carry the truncated signed distance, and free-space samples that carry
a sign only.  Loss: MisoLossMapping, L2 + free-space weights.

    python tools/pretrain_decoder_synthetic.py [--scenes 4] [--steps 300] [--points 65536] [--out decoder.pt]

Prints the loss every few steps, writes the decoder in the upstream state-dict format (network.{0,2,4}.weight / .bias),
then loads the file into a `fix: True` GridNet and queries it, to show that the frozen fused path accepts the result."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOUND = [[-1.0, 1.0], [-1.0, 1.0], [-1.0, 1.0]]
TRUNC = 0.15


def model_cfg(fix, pretrained=None, C=4, L=2, H=64):
    """the Newer College decoder shape: 2 levels of 4 features, 64 hidden units"""
    return {"name": "grid_net", "spatial_dim": 3,
            "decoder": {"type": "mlp", "hidden_dim": H, "hidden_layers": 1, "out_dim": 1, "pos_invariant": True,
                        "fix": fix, "pretrained_model": pretrained},
            "grid": {"type": "regular", "feature_dim": C, "init_stddev": 1e-2, "bound": BOUND, "base_cell_size": 0.2,
                     "per_level_scale": 2, "n_levels": L},
            "pose": {"optimize": False, "num_poses": 1}}


class Scene:
    """min over a few spheres, boxes and the plane z = floor of their signed distances (positive outside)"""

    def __init__(self, gen, dev):
        k = 3
        self.centres = (torch.rand(k, 3, generator=gen) * 1.2 - 0.6).to(dev)
        self.radii = (torch.rand(k, generator=gen) * 0.25 + 0.15).to(dev)
        self.box_c = (torch.rand(k, 3, generator=gen) * 1.2 - 0.6).to(dev)
        self.box_h = (torch.rand(k, 3, generator=gen) * 0.2 + 0.1).to(dev)
        self.floor = -0.8

    def sdf(self, p):
        d = (p[:, None, :] - self.centres[None]).norm(dim=-1) - self.radii[None]
        q = (p[:, None, :] - self.box_c[None]).abs() - self.box_h[None]
        box = q.clamp(min=0).norm(dim=-1) + q.max(dim=-1).values.clamp(max=0)
        return torch.cat((d, box, (p[:, 2:3] - self.floor)), dim=1).min(dim=1, keepdim=True).values

    def batch(self, n, gen_dev):
        """-> (model_input, gt) of MisoLossMapping: half the samples near the surface (uniform points pulled towards it
        along the numerical gradient), half anywhere; |sdf| < TRUNC is a valid distance, beyond it only the sign counts"""
        p = torch.rand(n, 3, device=self.centres.device, generator=gen_dev) * 1.9 - 0.95
        h = n // 2
        with torch.enable_grad():
            q = p[:h].clone().requires_grad_(True)
            d = self.sdf(q)
            g, = torch.autograd.grad(d.sum(), q)
        near = q.detach() - (d.detach() - (torch.rand(h, 1, device=p.device, generator=gen_dev) - 0.5) * 2 * TRUNC) * g
        p = torch.cat((near.clamp(-0.95, 0.95), p[h:]))
        d = self.sdf(p)
        valid = (d.abs() < TRUNC).float()
        sign = torch.where(d >= TRUNC, torch.ones_like(d), torch.zeros_like(d))
        gt = {"sdf": d.clamp(-TRUNC, TRUNC)[None], "sdf_valid": valid[None], "sdf_signs": sign[None]}
        mi = {"coords_frame": p[None], "sample_frame_ids": torch.zeros(1, n, 1, dtype=torch.int64, device=p.device),
              "weights": torch.ones(1, n, 1, device=p.device)}
        return mi, gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--points", type=int, default=65536)
    ap.add_argument("--lr", type=float, default=5e-3)
    ap.add_argument("--log-every", type=int, default=10)
    ap.add_argument("--out", type=str, default="decoder.pt")
    args = ap.parse_args()
    from miso_amd import ops
    from miso_amd.grid_opt.loss import MisoLossMapping
    from miso_amd.grid_opt.models.grid_net import GridNet
    dev = "cuda:0"
    torch.manual_seed(0)
    gen, gen_dev = torch.Generator().manual_seed(0), torch.Generator(device=dev).manual_seed(0)
    nets, scenes = [], []
    for s in range(args.scenes):
        net = GridNet(model_cfg(fix=False), device=dev).to(dev)
        net.set_initial_kf_pose(0, torch.eye(3), torch.zeros(3, 1), kf_key="KF0")
        net.unlock_feature()
        net.lock_pose()
        if nets:
            net.decoder = nets[0].decoder          # ONE decoder over all scenes
        nets.append(net)
        scenes.append(Scene(gen, dev))
    decoder = nets[0].decoder
    assert nets[0]._fused_decoder(trainable=True) is not None, "this decoder shape is not on the fused route"
    # L2 on the valid samples + the free-space bound on the rest, the weights of the reference's PretrainLoss
    lossf = MisoLossMapping(loss_type="L2", weight_sdf=3e3, weight_eik=0.0, weight_fs=100.0, trunc_dist=TRUNC)
    params = list(decoder.parameters()) + [g.feature for net in nets for g in net.features]
    opt = torch.optim.Adam(params, lr=args.lr)
    launches = []
    real = ops.sdf_wgrad_raw
    ops.sdf_wgrad_raw = lambda *a, **k: launches.append(1) or real(*a, **k)
    for step in range(args.steps):
        opt.zero_grad(set_to_none=True)
        total = 0.0
        for net, scene in zip(nets, scenes):
            mi, gt = scene.batch(args.points, gen_dev)
            loss = sum(lossf.compute(net, mi, gt).values())
            loss.backward()                        # the shared decoder's .grad adds up over the scenes
            total += float(loss.detach())
        opt.step()
        if step % args.log_every == 0 or step == args.steps - 1:
            print(f"step {step:5d} loss {total / args.scenes:.6f}", flush=True)
    ops.sdf_wgrad_raw = real
    assert len(launches) == args.steps * args.scenes, "the steps did not run the HIP weight-gradient kernel"
    decoder.save(args.out)
    print(f"wrote {args.out}: {sorted(decoder.state_dict())}")

    # the file in a frozen model: same grids, decoder loaded and fixed -> the frozen fused path, same values
    frozen = GridNet(model_cfg(fix=True, pretrained=args.out), device=dev).to(dev)
    with torch.no_grad():
        for a, b in zip(frozen.features, nets[0].features):
            a.feature.copy_(b.feature)
    pack = frozen._fused_decoder()
    assert pack is not None and not pack.trainable(), "the reloaded decoder did not take the frozen fused path"
    mi, gt = scenes[0].batch(args.points, gen_dev)
    with torch.no_grad():
        pred = frozen(mi["coords_frame"][0])
        trained = nets[0](mi["coords_frame"][0])
    valid = gt["sdf_valid"][0] == 1
    err = (pred - gt["sdf"][0])[valid].abs().mean().item()
    assert torch.equal(pred, trained)
    print(f"frozen fused path: ok (mean |sdf error| on near-surface samples of scene 0: {err:.4f} m)")


if __name__ == "__main__":
    main()
