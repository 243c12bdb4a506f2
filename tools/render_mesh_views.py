#!/usr/bin/env python3
"""Depth images of a triangle mesh from a list of camera poses: utils_sdf.render_mesh_depth per pose.

    python tools/render_mesh_views.py --mesh a.ply --poses poses.txt --out DIR [--width 640 --height 480 --fov 90]

``poses.txt`` is in KITTI format (utils_geometry.read_kitti_format_poses: twelve numbers per line, the row-major 3 x 4
camera-to-world pose, camera z forward, y down).  Writes DIR/depth_000000.npy ... (H, W) float32 z-depth in metres, 0
where nothing is hit, DIR/poses_kitti.txt (the poses as read) and DIR/camera.txt (fx fy cx cy H W).  The frames are what
PosedSdfRgbd.from_frames takes:
    depth = torch.from_numpy(np.stack([np.load(f) for f in sorted(glob('DIR/depth_*.npy'))]))
    PosedSdfRgbd.from_frames(depth, R, t, cam)
On a HIP device the rays go through ops.MeshIndex (csrc/mesh.hip), built once; with --device cpu through
utils_geometry.cast_rays_torch."""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", required=True)
    ap.add_argument("--poses", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--fov", type=float, default=90.0, help="horizontal field of view, degrees")
    ap.add_argument("--max-dist", type=float, default=50.0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    from miso_amd.grid_opt.utils import utils_geometry, utils_sdf
    from miso_amd.grid_opt.utils.utils_data import CameraParameters
    poses = utils_geometry.read_kitti_format_poses(args.poses)
    if not poses:
        raise SystemExit(f"{args.poses}: no KITTI-format poses")
    f = 0.5 * args.width / math.tan(0.5 * math.radians(args.fov))
    cam = CameraParameters(fx=f, fy=f, cx=0.5 * args.width - 0.5, cy=0.5 * args.height - 0.5, H=args.height, W=args.width)
    device = torch.device(args.device)
    mesh = utils_sdf.read_ply(args.mesh)
    if device.type == "cuda":
        from miso_amd import ops
        verts, tris = utils_sdf._mesh_arrays(mesh, device)
        mesh = ops.MeshIndex(verts, tris)
        print(f"{args.mesh}: {mesh.n_tri} triangles, grid {mesh.stats()}")
    os.makedirs(args.out, exist_ok=True)
    for k, T in enumerate(poses):
        R = torch.tensor(T[:3, :3], dtype=torch.float32, device=device)
        t = torch.tensor(T[:3, 3], dtype=torch.float32, device=device)
        depth, mask = utils_sdf.render_mesh_depth(mesh, R, t, cam, max_dist=args.max_dist)
        np.save(os.path.join(args.out, f"depth_{k:06d}.npy"), depth.cpu().numpy())
        print(f"pose {k}: {int(mask.sum())} of {mask.numel()} pixels hit")
    utils_geometry.write_kitti_format_poses(os.path.join(args.out, "poses_kitti.txt"), np.stack(poses), direct_use_filename=True)
    with open(os.path.join(args.out, "camera.txt"), "w") as fh:
        fh.write(f"{cam.fx} {cam.fy} {cam.cx} {cam.cy} {cam.H} {cam.W}\n")


if __name__ == "__main__":
    main()
