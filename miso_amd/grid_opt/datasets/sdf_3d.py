"""SDF samples of a mesh (reference: grid_opt/datasets/sdf_3d.py): ``Sdf3D`` / ``BatchedSdf3D`` (:17-155, :417-447), samples
everywhere in the volume labelled with the mesh's signed distance, and ``PosedSdf3D`` / ``BatchPosedSdf3D`` (:157-383,
:449-495), samples along the rays of simulated camera views.

The reference gets the signed distance from pysdf and the ray casts from Open3D's RaycastingScene.  Here both come from
the mesh index: ``utils_sdf.MeshSdf`` (``ops.MeshIndex.closest`` / ``contains``, csrc/mesh_sdf.hip, on a HIP device;
``utils_geometry.closest_on_mesh_torch`` / ``count_crossings_torch`` on the CPU) is the pysdf-shaped callable, positive
inside, and the rays of a frame go through ONE cast (``ops.MeshIndex.cast_rays`` / ``utils_geometry.cast_rays_torch``).
The random draws come from numpy's global generator on the host, in the reference's order, and are then moved: the CPU
and the device route draw the same numbers from the same seed.  (``Sdf3D``'s surface samples come from
``utils_eval.sample_points_from_mesh``, seeded from that generator: not trimesh's stream.)

``PosedSdf3D`` meets the signed distance twice:
  * cameras are placed where sdf > 0.3 (:193-199).  ``sdf_fn='mesh'`` runs that loop against the dataset's own mesh; a
    callable ``sdf_fn`` (points (N, 3) numpy -> (N,) distances, positive inside, pysdf's call) against the caller's;
    ``frame_poses`` = (R (F, 3, 3), t (F, 3, 1)) are used as given; with none of the three the constructor raises.
  * hit points are labelled sdf_fn(point) (:252): with 'mesh' on the device, no host round trip.  Without ``sdf_fn`` they
    are labelled 0 and valid: they lie on the surface up to the cast's rounding.
``visualize_open3d`` is left out, as elsewhere."""
import logging
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from miso_amd.grid_opt.utils import utils_geometry, utils_sample
from miso_amd.grid_opt.utils.utils_sdf import MeshSdf, TriangleMesh, read_ply

logger = logging.getLogger(__name__)


class Sdf3D(Dataset):
    """Samples with the true signed distance everywhere: on the surface, in free space and inside (reference :17-155).
    The reference's arguments, and ``device`` of the samples and batches.  Of ``total_samples`` (a multiple of 8) the first
    half lies on the surface and is labelled 0 without a query, three eighths are surface samples moved by a Gaussian of
    ``surface_stddev``, one eighth is uniform in the bound; the SDF is MeshSdf's, positive inside, not negated, as there.
    ``trunc_dist``: a sample is valid while |sdf| < trunc_dist, and beyond it only the sign is kept (sdf_sign = +-1)."""

    def __init__(self, meshfile, batch_size=2 ** 16, total_samples=2 ** 20, normalize=False, surface_stddev=0.1, bound_buffer=0.5,
                 trunc_dist=None, *, device='cuda:0'):
        super().__init__()
        self.meshfile = meshfile
        mesh = meshfile if isinstance(meshfile, TriangleMesh) else read_ply(os.fspath(meshfile))
        v = np.asarray(mesh.vertices, dtype=np.float64)
        self.normalize = normalize
        if normalize:                                           # into [-1, 1]: centre of the box, 0.95 of its diagonal
            vmin, vmax = v.min(axis=0), v.max(axis=0)
            self.v_scale = 2.0 / np.sqrt(np.sum((vmax - vmin) ** 2)) * 0.95
            mesh = TriangleMesh((v - (vmin + vmax)[None, :] / 2.0) * self.v_scale, mesh.triangles)
            self.bound = np.array([[-1.0, 1.0]] * 3)
            self.surface_stddev = 0.01
        else:
            self.bound = np.stack([v.min(axis=0) - bound_buffer, v.max(axis=0) + bound_buffer], axis=1)     # (3, 2)
            self.surface_stddev = surface_stddev
        self.mesh = mesh
        if not _is_watertight(mesh.triangles):
            logger.warning("the mesh is not closed (some edge is not shared by exactly two triangles): the sign of its "
                           "distance is a crossing parity and may be wrong")
        self.device = torch.device(device)
        self.sdf_fn = MeshSdf(mesh.vertices, mesh.triangles, device=self.device)
        self.total_samples, self.batch_size, self.trunc_dist = total_samples, batch_size, trunc_dist
        assert self.total_samples % 8 == 0, "total_samples must be divisible by 8."
        self.resample()

    def __len__(self):
        return self.total_samples // self.batch_size + 1

    def _sample_uniformly(self, k):
        return np.stack([np.random.uniform(self.bound[a, 0], self.bound[a, 1], k) for a in range(3)], axis=1)

    def resample(self):
        from miso_amd.grid_opt.utils import utils_eval
        n, half = self.total_samples, self.total_samples // 2
        surface = utils_eval.sample_points_from_mesh(self.mesh, n * 7 // 8, voxel_down_sample_res=0.0,
                                                     seed=int(np.random.randint(0, 2 ** 31 - 1)))
        surface[half:] += self.surface_stddev * np.random.randn(n * 3 // 8, 3)
        points = np.concatenate([surface, self._sample_uniformly(n // 8)], axis=0).astype(np.float32)
        self.coords = torch.from_numpy(points).to(self.device)
        sdfs = torch.zeros((n, 1), dtype=torch.float32, device=self.device)
        sdfs[half:, 0] = self.sdf_fn.on_device(self.coords[half:])
        finite = sdfs.abs() < 1e10                              # (a mesh without a triangle answers +inf)
        valid, signs = finite, torch.zeros_like(sdfs)
        if self.trunc_dist is not None:
            assert self.trunc_dist > 0
            valid = sdfs.abs() < self.trunc_dist
            signs = torch.where(finite & (sdfs > self.trunc_dist), 1.0, 0.0) - torch.where(finite & (sdfs < -self.trunc_dist), 1.0, 0.0)
        self.sdfs, self.sdf_valid, self.sdf_signs = sdfs, valid.float(), signs.float()

    def __getitem__(self, idx):
        pick = torch.from_numpy(np.random.choice(self.total_samples, size=self.batch_size)).to(self.device)
        return {'coords': self.coords[pick]}, {'sdf': self.sdfs[pick], 'sdf_valid': self.sdf_valid[pick],
                                               'sdf_sign': self.sdf_signs[pick]}

    def get_inflated_bound(self):
        assert not self.normalize
        return self.bound


def _is_watertight(triangles) -> bool:
    """every undirected edge belongs to exactly two triangles"""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    if not len(t):
        return False
    edges = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    return bool((np.unique(edges, axis=0, return_counts=True)[1] == 2).all())


class BatchedSdf3D(Dataset):
    """A collection of Sdf3D datasets, one per mesh (reference :417-447); a batch comes from one of them at random and
    carries its ``dataset_index``."""

    def __init__(self, filelist, batch_size=2 ** 16, total_samples=2 ** 20, normalize=False, surface_stddev=0.1, trunc_dist=None,
                 *, device='cuda:0'):
        super().__init__()
        self.num_datasets = len(filelist)
        self.datasets = [Sdf3D(meshfile, batch_size=batch_size, total_samples=total_samples, normalize=normalize,
                               surface_stddev=surface_stddev, trunc_dist=trunc_dist, device=device) for meshfile in filelist]
        self.len = sum(len(d) for d in self.datasets)

    def __len__(self):
        return self.len

    def __getitem__(self, idx):
        dataset_index = np.random.choice(self.num_datasets, size=1)[0]
        dataset = self.datasets[dataset_index]
        input_dict, gt_dict = dataset[np.random.choice(len(dataset), size=1)[0]]
        input_dict['dataset_index'] = torch.tensor(dataset_index).long()
        return input_dict, gt_dict


class PosedSdf3D(Dataset):
    """A SDF dataset obtained by simulating random camera views (reference :157-383).  The reference's arguments, and:
    ``device`` of the frames and batches; ``frame_poses`` / ``sdf_fn`` (module docstring: 'mesh', a callable or None); ``meshfile`` may be a
    TriangleMesh; ``fov_deg`` / ``width_px`` / ``height_px`` of the simulated camera (the reference hard-wires 90, 640, 480)."""

    def __init__(self, meshfile, frame_batchsize=2 ** 14, frame_samples=2 ** 14, num_frames=64, near_surface_n=2,
                 near_surface_std=0.05, free_space_n=1, trunc_dist=0.15, frame_std_rad=0.0, frame_std_meter=0.0,
                 distance_std=0.0, *, device='cuda:0', frame_poses=None, sdf_fn=None, fov_deg=90.0, width_px=640,
                 height_px=480):
        super().__init__()
        self.meshfile = meshfile
        self.mesh = meshfile if isinstance(meshfile, TriangleMesh) else read_ply(os.fspath(meshfile))
        v = np.asarray(self.mesh.vertices, dtype=np.float64)
        self.bound = np.stack([v.min(axis=0), v.max(axis=0)], axis=1)                  # (3, 2)
        self.near_surface_std, self.near_surface_n = near_surface_std, near_surface_n
        self.free_space_n, self.trunc_dist = free_space_n, trunc_dist
        self.frame_std_rad, self.frame_std_meter, self.distance_std = frame_std_rad, frame_std_meter, distance_std
        self.frame_samples, self.frame_batchsize = frame_samples, frame_batchsize
        self.device = torch.device(device)
        if isinstance(sdf_fn, str):
            if sdf_fn != 'mesh':
                raise ValueError(f"sdf_fn = {sdf_fn!r}: 'mesh' (the dataset's own mesh), a callable, or None")
            sdf_fn = MeshSdf(self.mesh.vertices, self.mesh.triangles, device=self.device)
        self.sdf_fn = sdf_fn
        self.fov_deg, self.width_px, self.height_px = float(fov_deg), int(width_px), int(height_px)
        if frame_poses is not None:
            R, t = frame_poses
            self.R_world_frame_gt = torch.as_tensor(R, dtype=torch.float32).reshape(-1, 3, 3).clone()
            self.t_world_frame_gt = torch.as_tensor(t, dtype=torch.float32).reshape(-1, 3, 1).clone()
            self.num_frames = int(self.R_world_frame_gt.shape[0])
        elif sdf_fn is not None:
            self.num_frames = num_frames
            self.R_world_frame_gt = utils_geometry.wrapped_gaussian_rotations(num_frames, std_rad=1.0)
            t_gt = np.zeros((num_frames, 3, 1))
            for frame_id in range(num_frames):                  # a camera sits properly in free space (reference :193-199)
                while True:
                    position = utils_geometry.uniform_translations(1, self.bound)
                    sdf = float(np.asarray(sdf_fn(position.numpy()), dtype=np.float32).reshape(-1)[0])
                    if 0.3 < sdf < 1e10:
                        break
                t_gt[frame_id, :, 0] = position.numpy().flatten()
            self.t_world_frame_gt = torch.from_numpy(t_gt).float()
        else:
            raise ValueError("PosedSdf3D places its cameras where the mesh's signed distance exceeds 0.3, and the signed "
                             "distance to a mesh (pysdf in the reference) is not built here unless asked for: give "
                             "sdf_fn='mesh', frame_poses=(R, t), or sdf_fn, a callable returning the mesh signed distance "
                             "of (N, 3) points")
        self.R_world_frame_gt = self.R_world_frame_gt.to(self.device)
        self.t_world_frame_gt = self.t_world_frame_gt.to(self.device)
        self.sample_frames()
        self.resample_poses()

    def __len__(self):
        return (1 + self.free_space_n + self.near_surface_n) * self.frame_samples // self.frame_batchsize

    def _caster(self):
        """rays (N, 6) -> t (N,), by the route of this dataset's device; built once for all frames"""
        verts = torch.as_tensor(np.asarray(self.mesh.vertices), dtype=torch.float32, device=self.device)
        tris = torch.as_tensor(np.asarray(self.mesh.triangles), dtype=torch.int64, device=self.device)
        if self.device.type == 'cuda':
            from miso_amd import ops
            own = isinstance(self.sdf_fn, MeshSdf) and isinstance(self.sdf_fn.mesh, ops.MeshIndex)
            index = self.sdf_fn.mesh if own else ops.MeshIndex(verts, tris)       # sdf_fn='mesh': one index for both
            return lambda rays: index.cast_rays(rays[:, :3], rays[:, 3:])[0]
        chunk = max(1, min(4096, (1 << 22) // max(int(tris.shape[0]), 1)))
        return lambda rays: utils_geometry.cast_rays_torch(rays[:, :3], rays[:, 3:], verts, tris, chunk=chunk)[0]

    def _draw(self, array):
        return torch.from_numpy(np.ascontiguousarray(array)).to(device=self.device, dtype=torch.float32)

    def sample_frames(self):
        """One cast per frame, then parts I-III of the reference's sample_frames (:209-312) as tensor ops on the device."""
        cast = self._caster()
        self.frames = []
        for frame_id in range(self.num_frames):
            twf, Rwf = self.t_world_frame_gt[frame_id], self.R_world_frame_gt[frame_id]
            eye = twf.reshape(3)
            center = eye - Rwf[:, 2]                           # the camera looks down its negative z axis (:223)
            rays = utils_sample.pinhole_rays_lookat(self.fov_deg, center, eye, Rwf[:, 1], self.width_px, self.height_px,
                                                    device=self.device)
            t_hit = cast(rays)
            hit = torch.isfinite(t_hit).nonzero().flatten()
            n_hit = int(hit.numel())
            assert n_hit > 0, f"Frame {frame_id} has no hit point!"
            # Part I: intersection points
            n_keep = min(self.frame_samples, n_hit)
            keep = hit[torch.from_numpy(np.random.permutation(n_hit)[:n_keep]).to(self.device)]
            points_gt = rays[keep, :3] + rays[keep, 3:] * t_hit[keep, None]
            if isinstance(self.sdf_fn, MeshSdf):                # labelled where the points are
                sdfs = self.sdf_fn.on_device(points_gt.contiguous()).reshape(-1, 1)
                sdfs_valid = (sdfs.abs() < 1e10).float()
            elif self.sdf_fn is not None:
                sdfs = self._draw(np.asarray(self.sdf_fn(points_gt.cpu().numpy()), dtype=np.float32).reshape(-1, 1))
                sdfs_valid = (sdfs.abs() < 1e10).float()
            else:                                               # on the surface: 0 and valid (module docstring)
                sdfs, sdfs_valid = torch.zeros(n_keep, 1, device=self.device), torch.ones(n_keep, 1, device=self.device)
            dist_gt = (points_gt - eye).norm(dim=1, keepdim=True).clamp(min=1e-6)
            dir_gt = (points_gt - eye) / dist_gt
            points_hit = eye + dir_gt * (dist_gt + self._draw(np.random.randn(n_keep, 1)) * self.distance_std)
            points, labels, valid, signs = [points_hit], [sdfs], [sdfs_valid], [torch.zeros(n_keep, 1, device=self.device)]
            # Part II: near-surface samples along the ray
            dist = (points_hit - eye).norm(dim=1, keepdim=True).clamp(min=1e-6)
            direction = (points_hit - eye) / dist
            rep_dist = dist.repeat_interleave(self.near_surface_n, dim=0)
            rep_dir = direction.repeat_interleave(self.near_surface_n, dim=0)
            disp = self._draw(np.random.randn(n_keep * self.near_surface_n, 1)) * self.near_surface_std
            points.append(eye + rep_dir * (rep_dist + disp))
            labels.append(-disp)
            valid.append(torch.ones_like(disp))
            signs.append(torch.zeros_like(disp))
            # Part III: free-space samples, outside the truncation region
            rep_dist = dist.repeat_interleave(self.free_space_n, dim=0)
            rep_dir = direction.repeat_interleave(self.free_space_n, dim=0)
            ratio = 0.01 + self._draw(np.random.rand(n_keep * self.free_space_n, 1)) * (0.99 - 0.01)
            disp = torch.clamp((ratio - 1.0) * rep_dist, max=-self.trunc_dist)
            points.append(eye + rep_dir * (rep_dist + disp))
            labels.append(-disp)
            valid.append(torch.zeros_like(disp))
            signs.append(torch.ones_like(disp))
            # Part IV: assemble
            points_world = torch.cat(points, dim=0)
            self.frames.append({
                'R_world_frame_gt': Rwf, 't_world_frame_gt': twf,
                'points_frame': utils_geometry.transfrom_points_from(points_world, Rwf, twf),
                'sdfs': torch.cat(labels, dim=0), 'sdfs_valid': torch.cat(valid, dim=0), 'signs': torch.cat(signs, dim=0)})

    def resample_poses(self):
        """noisy pose estimates; the first pose is not perturbed (reference :314-326)"""
        t_noise = utils_geometry.gaussian_translations(self.num_frames, stddev=self.frame_std_meter).unsqueeze(-1)
        R_noise = utils_geometry.wrapped_gaussian_rotations(self.num_frames, std_rad=self.frame_std_rad)
        t_noise[0, :] = 0.0
        R_noise[0, :, :] = torch.eye(3)
        self.t_world_frame = self.t_world_frame_gt + t_noise.to(self.device)
        self.R_world_frame = torch.matmul(self.R_world_frame_gt, R_noise.to(self.device))
        for frame_id in range(self.num_frames):
            self.frames[frame_id]['R_world_frame'] = self.R_world_frame[frame_id]
            self.frames[frame_id]['t_world_frame'] = self.t_world_frame[frame_id]

    def true_kf_pose_in_world(self, kf_id):
        return self.R_world_frame_gt[kf_id], self.t_world_frame_gt[kf_id]

    def noisy_kf_pose_in_world(self, kf_id):
        return self.R_world_frame[kf_id], self.t_world_frame[kf_id]

    def __getitem__(self, index):
        cols = {k: [] for k in ('frame', 'noisy', 'gt', 'sdf', 'valid', 'sign')}
        spans, begin = [], 0
        for frame_id, frame in enumerate(self.frames):
            size = int(frame['points_frame'].shape[0])
            count = min(self.frame_batchsize, size)
            pick = torch.from_numpy(np.random.choice(size, size=count)).to(self.device)
            pts = frame['points_frame'][pick]
            cols['frame'].append(pts)
            cols['sdf'].append(frame['sdfs'][pick])
            cols['valid'].append(frame['sdfs_valid'][pick])
            cols['sign'].append(frame['signs'][pick])
            cols['noisy'].append(utils_geometry.transform_points_to(pts, self.R_world_frame[frame_id], self.t_world_frame[frame_id]))
            cols['gt'].append(utils_geometry.transform_points_to(pts, self.R_world_frame_gt[frame_id],
                                                                 self.t_world_frame_gt[frame_id]))
            spans.append([begin, begin + count])
            begin += count
        input_dict = {'R_world_frame': self.R_world_frame, 't_world_frame': self.t_world_frame,
                      'coords_frame': torch.cat(cols['frame'], dim=0), 'coords_world_noisy': torch.cat(cols['noisy'], dim=0),
                      'coords_world_gt': torch.cat(cols['gt'], dim=0),
                      'frame_indices': torch.tensor(spans, dtype=torch.long, device=self.device).reshape(-1, 2)}
        gt_dict = {'sdf': torch.cat(cols['sdf'], dim=0), 'sdf_valid': torch.cat(cols['valid'], dim=0),
                   'sdf_signs': torch.cat(cols['sign'], dim=0), 'R_world_frame_gt': self.R_world_frame_gt,
                   't_world_frame_gt': self.t_world_frame_gt}
        return input_dict, gt_dict

    def get_inflated_bound(self):
        return np.concatenate((self.bound[:, :1] - 0.5, self.bound[:, 1:] + 0.5), axis=1)


class BatchPosedSdf3D(Dataset):
    """A collection of PosedSdf3D datasets, one per mesh (reference :449-495).  ``frame_poses`` / ``sdf_fn``: one entry per
    mesh, or None; ``sdf_fn='mesh'``: every dataset's own mesh."""

    def __init__(self, filelist, frame_batchsize=2 ** 14, frame_samples=2 ** 14, num_frames=64, near_surface_n=2,
                 near_surface_std=0.05, free_space_n=1, trunc_dist=0.15, frame_std_rad=0.0, frame_std_meter=0.0,
                 distance_std=0.0, resample_poses_freq=None, *, device='cuda:0', frame_poses=None, sdf_fn=None, **camera):
        super().__init__()
        self.num_datasets = len(filelist)
        self.len = 0
        self.datasets = []
        for i, meshfile in enumerate(filelist):
            dataset = PosedSdf3D(meshfile, frame_batchsize=frame_batchsize, frame_samples=frame_samples, num_frames=num_frames,
                                 near_surface_n=near_surface_n, near_surface_std=near_surface_std, free_space_n=free_space_n,
                                 trunc_dist=trunc_dist, frame_std_rad=frame_std_rad, frame_std_meter=frame_std_meter,
                                 distance_std=distance_std, device=device,
                                 frame_poses=None if frame_poses is None else frame_poses[i],
                                 sdf_fn=sdf_fn if sdf_fn is None or isinstance(sdf_fn, str) else sdf_fn[i], **camera)
            self.len += len(dataset)
            self.datasets.append(dataset)
        self.getitem_count = 0
        self.resample_poses_freq = resample_poses_freq

    def __len__(self):
        return self.len

    def __getitem__(self, idx):
        self.getitem_count += 1
        if self.resample_poses_freq is not None and self.getitem_count % self.resample_poses_freq == 0:
            self.resample_poses()
        dataset_index = np.random.choice(self.num_datasets, size=1)[0]
        dataset = self.datasets[dataset_index]
        inner_index = np.random.choice(len(dataset), size=1)[0]
        input_dict, gt_dict = dataset[inner_index]
        input_dict['dataset_index'] = torch.tensor(dataset_index).long()
        input_dict['dataset_bound'] = torch.from_numpy(dataset.get_inflated_bound()).float()
        return input_dict, gt_dict

    def resample_poses(self):
        logger.info("Resample noisy poses!")
        for dataset in self.datasets:
            dataset.resample_poses()
