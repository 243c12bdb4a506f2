"""Generate tests/golden/voxel_down.npz by IMPORTING the reference (MISO) on the CPU.

What is recorded, on the seeded clouds of tests/voxel_cases.py (index arrays only):
  idx_<case>        what the reference's utils_geometry.voxel_down_sample_torch returns for the case
  lidar_kept_<f>    the rows of LiDAR frame f that survive the reference's load sequence (adaptive crop range, adapted
                    voxel size, its voxel_down_sample_torch, its crop_points), as indices into the frame

    python tools/make_voxel_goldens.py

Needs the reference checkout (MISO_REFERENCE, see tools/make_goldens.py); only the fixture is committed.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens import ROOT, import_reference  # noqa: E402


def adaptive_range(pts: np.ndarray, max_range: float) -> np.float32:
    """Twice the larger of the frame's smaller |x| and smaller |y| extent, capped at max_range (fp32 throughout)."""
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    nearer = [np.minimum(np.abs(hi[a]), np.abs(lo[a])) for a in (0, 1)]
    return np.minimum(np.float32(max_range), np.float32(2.0) * np.maximum(*nearer))


def main():
    import_reference()
    import grid_opt.utils.utils_geometry as rgeom
    import voxel_cases as vc
    out = {}
    for name, (pts, v) in vc.cases().items():
        out[f"idx_{name}"] = rgeom.voxel_down_sample_torch(torch.from_numpy(pts), v).numpy().astype(np.int64)
        print(name, pts.shape[0], "->", out[f"idx_{name}"].shape[0])
    c = vc.LIDAR
    for f, pts in enumerate(vc.lidar_frames()):
        crop_range = adaptive_range(pts, c["max_range"])
        voxel = torch.tensor(crop_range) / c["max_range"] * c["voxel_size"]          # a 0-dim fp32 tensor, as upstream
        keep = rgeom.voxel_down_sample_torch(torch.from_numpy(pts), voxel)
        _, kept = rgeom.crop_points(torch.from_numpy(pts)[keep], keep, c["min_z"], c["max_z"], c["min_range"],
                                    torch.tensor(crop_range))
        out[f"lidar_kept_{f}"] = kept.numpy().astype(np.int64)
        print("lidar", f, pts.shape[0], "->", keep.shape[0], "->", kept.shape[0], "range", float(crop_range),
              "voxel", float(voxel))
    path = os.path.join(ROOT, "tests", "golden", "voxel_down.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
