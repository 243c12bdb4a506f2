"""Grade a reconstructed mesh against a ground-truth one: the sequence that ends the reference's flagship demo
(demo/full_slam_scannet.py:161-191, grid_opt/utils/utils_ncd.py:121-128):

    sample_points_from_mesh (both)  ->  crop the prediction to the ground truth's box  ->  compute_chamfer_metrics

    python tools/eval_mesh.py --pred a.ply --gt b.ply [--threshold 0.05 --voxel 0.02 --points 1000000
                                                       --crop pca|aabb|none --align --normals faces|knn
                                                       --out metrics.json]

--align: utils_scannet.align_mesh_to_ref moves the prediction onto the ground truth first (coarse and fine ICP, the
demo's second step), so that a pose offset of the reconstruction is not graded as surface error; off by default.
--normals: the target normals of that ICP, the sampled faces' (default) or, as upstream, estimated from the samples'
30 nearest neighbours.

--crop pca: an OrientedBox along the principal axes of the ground-truth samples (not Open3D's minimal box); aabb: their
axis-aligned box; both grown by --crop_buffer.  The nearest-neighbour search runs on the HIP device (ops.nearest)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from miso_amd.grid_opt.utils import utils_eval  # noqa: E402


def evaluate(pred, gt, threshold=0.05, voxel=0.02, points=1000000, crop='pca', crop_buffer=0.05, seed=0, align=False,
             normals='faces'):
    """pred, gt: PLY paths or TriangleMesh objects -> (metrics dict, number of prediction points, of ground-truth points)"""
    if align:
        from miso_amd.grid_opt.utils import utils_scannet
        pred, icp = utils_scannet.align_mesh_to_ref(pred, gt, voxel_size=voxel if voxel > 0 else 0.02, num_points=points,
                                                    seed=seed, normals=normals)
        print(f"aligned: {icp}")
    verts_pred = utils_eval.sample_points_from_mesh(pred, mesh_sample_point=points, voxel_down_sample_res=voxel, seed=seed)
    verts_trgt = utils_eval.sample_points_from_mesh(gt, mesh_sample_point=points, voxel_down_sample_res=voxel,
                                                    seed=seed + 1)
    if crop == 'pca':
        verts_pred = utils_eval.filter_points_by_oriented_bound(
            verts_pred, utils_eval.OrientedBox.from_points(verts_trgt, buffer=crop_buffer))
    elif crop == 'aabb':
        lo, hi = verts_trgt.min(axis=0) - crop_buffer, verts_trgt.max(axis=0) + crop_buffer
        verts_pred = utils_eval.filter_points_by_bound(verts_pred, np.stack([lo, hi], axis=1))
    elif crop != 'none':
        raise ValueError(f"unknown --crop {crop}")
    metrics = utils_eval.compute_chamfer_metrics(verts_pred, verts_trgt, threshold=threshold, truncation_acc=0.50,
                                                 truncation_com=0.50)
    return metrics, len(verts_pred), len(verts_trgt)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--pred', required=True, help='the reconstructed mesh (PLY)')
    ap.add_argument('--gt', required=True, help='the ground-truth mesh (PLY)')
    ap.add_argument('--threshold', type=float, default=0.05, help='precision / recall distance, metres')
    ap.add_argument('--voxel', type=float, default=0.02, help='centroid down-sample of both clouds, metres (0: off)')
    ap.add_argument('--points', type=int, default=1000000, help='surface samples per mesh')
    ap.add_argument('--crop', choices=('pca', 'aabb', 'none'), default='pca')
    ap.add_argument('--crop_buffer', type=float, default=0.05)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--align', action='store_true', help='ICP the prediction onto the ground truth before sampling')
    ap.add_argument('--normals', choices=('faces', 'knn'), default='faces', help="--align's target normals")
    ap.add_argument('--out', type=str, default=None, help='write the metrics as JSON')
    args = ap.parse_args(argv)
    metrics, n_pred, n_gt = evaluate(args.pred, args.gt, args.threshold, args.voxel, args.points, args.crop,
                                     args.crop_buffer, args.seed, args.align, args.normals)
    print(f"{n_pred} prediction points, {n_gt} ground-truth points")
    print(json.dumps({k: round(float(v), 6) for k, v in metrics.items()}, indent=4))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump({k: float(v) for k, v in metrics.items()}, f, indent=4)
    return metrics


if __name__ == "__main__":
    main()
